"""Ray-cast surfaces on the host: the rules of include/supnerf_hip.h ("Ray-cast surfaces") as tests/ray_restatement.py restates them, run
in float32 on the oracle decoder with the planted box and judged against a float64 truth (a 4001-sample float64 march, then bisection);
the implicit-function gradient of rule 8 against a central difference of that truth; and the parts of the new API that need no GPU
(symbols, signatures, argument checks, the frame maps)."""
import inspect

import numpy as np
import pytest
import torch

import ray_restatement as RR
from geometry_cases import LEVEL_BOX
from oracle import supnerf_oracle as O
from planted_decoder import HALF, WOBBLE, box_rays, planted_params

NEAR, FAR, S = 0.75, 2.25, 64
REFINES = [(0, 2), (8, 3), (4, 5), (2, 17), (1, 257), (3, 17)]


def _code(seed=5, B=1):
    return torch.randn(B, 256, generator=torch.Generator().manual_seed(seed)) * 0.5


@pytest.fixture(scope="module")
def box_case():
    """The planted box with wobble, one code, 512 rays (the first 128 aimed past the box), the float32 and float64 density callables and
    the float64 truth."""
    p32 = planted_params(3, 1, seed=1, wobble=WOBBLE)
    p64 = {k: v.double() for k, v in p32.items()}
    code = _code()
    o, d, _ = box_rays(512, 64, seed=3)
    f32, f64 = RR.oracle_sigma_fn(p32, code), RR.oracle_sigma_fn(p64, code)
    state, depth = RR.truth(f64, o.numpy(), d.numpy(), NEAR, FAR, LEVEL_BOX)
    return dict(p32=p32, p64=p64, code=code, o=o.numpy(), d=d.numpy(), f32=f32, f64=f64, state=state, depth=depth)


def test_oracle_sigma_is_the_oracle_decoders_sigma():
    p = planted_params(3, 1, seed=1, wobble=WOBBLE)
    g = torch.Generator().manual_seed(2)
    xyz = (torch.rand(2 * 50, 3, generator=g) - 0.5) * 1.4
    sc = _code(7, 2)
    want, _ = O.decoder_forward(p, xyz.view(-1, 1, 3), torch.zeros(100, 1, 3), sc, torch.zeros_like(sc))
    assert torch.equal(RR.oracle_sigma(p, xyz, sc), want.view(-1))
    # (the callable runs object by object: another GEMM blocking on the host, so equal to rounding, not to the bit)
    assert np.allclose(RR.oracle_sigma_fn(p, sc)(xyz.numpy()), want.view(-1).numpy(), rtol=1e-4, atol=1e-30)


def test_march_ends_are_exact_and_a_sub_march_reproduces_its_bracket(box_case):
    """Rule 1: the first and last sample of a march are ta and tb bit for bit, for any (ta, tb, S); so a refinement march evaluates the
    decoder at its bracket's two end points again and finds (va, vb) bit for bit."""
    g = np.random.default_rng(0)
    for S_ in (2, 3, 5, 17, 37, 64, 200, 257):
        ta = g.uniform(-3, 3, 4000).astype(np.float32)
        tb = (ta + g.uniform(0, 2, 4000).astype(np.float32) * np.float32(10.0) ** g.integers(-6, 1, 4000).astype(np.float32)).astype(np.float32)
        tb[:10] = ta[:10]
        t = RR.march_t(ta, tb, S_)
        assert t.dtype == np.float32 and np.array_equal(t[:, 0], ta) and np.array_equal(t[:, -1], tb)
        assert (np.diff(t.astype(np.float64), axis=1) >= 0).all()                 # monotone (ties in a narrow bracket), never past tb
    c = box_case
    first = RR.ray_surface(c["f32"], c["o"], c["d"], NEAR, FAR, LEVEL_BOX, S)
    hit = first["state"] == 1
    for s_r in (3, 17):
        pts = RR.march_points(c["o"], c["d"], first["ta"], first["tb"], s_r)
        sig = c["f32"](pts).reshape(-1, s_r)
        assert np.array_equal(sig[hit, 0], first["va"][hit]) and np.array_equal(sig[hit, -1], first["vb"][hit])
        assert (sig[hit, 0] < LEVEL_BOX).all() and (sig[hit, -1] >= LEVEL_BOX).all()


@pytest.mark.parametrize("refine", REFINES)
def test_states_and_depths_against_the_float64_truth(box_case, refine):
    """Every one of the 512 rays has the truth's state (384 hits, 128 misses), no state-1 ray loses its crossing in a refinement, every
    depth lies in its final bracket together with the truth (|t - truth| <= width), and the bracket has shrunk as the rule says: width <=
    1.01 (far - near) / (S - 1) / (S_r - 1)^levels, the 1 % being room for the fp32 rounding of the sample positions."""
    c = box_case
    assert int((c["state"] == 1).sum()) == 384 and int((c["state"] == 0).sum()) == 128 and not (c["state"] == 2).any()
    assert (c["state"][:128] == 0).all()
    r = RR.ray_surface(c["f32"], c["o"], c["d"], NEAR, FAR, LEVEL_BOX, S, refine)
    assert np.array_equal(r["state"], c["state"])
    assert r["lost"] == 0
    hit = r["state"] == 1
    t, w, truth = r["depth"].astype(np.float64), r["width"].astype(np.float64), c["depth"]
    err = np.abs(t - truth)[hit]
    bound = 1.01 * (FAR - NEAR) / (S - 1) / (refine[1] - 1) ** refine[0]
    print(f"refine {refine}: max |t - truth| {err.max():.3e}, max width {w[hit].max():.4e} (bound {bound:.4e})")
    assert (err <= w[hit]).all()
    assert (r["depth"][hit] >= r["ta"][hit]).all() and (r["depth"][hit] <= r["tb"][hit]).all()
    assert (truth[hit] >= r["ta"][hit]).all() and (truth[hit] <= r["tb"][hit]).all()
    assert w[hit].max() <= bound
    assert (r["depth"][~hit] == 0).all() and (r["width"][~hit] == 0).all()


def test_rays_that_start_inside(box_case):
    """State 2: sigma at near is already inside.  Depth = near, width 0, and rule 8 gives exactly zero."""
    c = box_case
    g = torch.Generator().manual_seed(4)
    o = ((torch.rand(32, 3, generator=g) * 2 - 1) * torch.tensor(HALF) * 0.5).numpy()
    d = torch.nn.functional.normalize(torch.randn(32, 3, generator=g), dim=1).numpy()
    near = np.full(32, 0.0, np.float32)
    near[16:] = 0.01
    for refine in ((0, 2), (2, 17)):
        r = RR.ray_surface(c["f32"], o, d, near, 2.0, LEVEL_BOX, 16, refine)
        assert (r["state"] == 2).all() and np.array_equal(r["depth"], near) and (r["width"] == 0).all()
        assert np.array_equal(r["ta"], near) and np.array_equal(r["tb"], near)
        gx = torch.randn(32, 3, generator=g)
        d_o, d_d, cc = RR.implicit_gradient(gx, torch.from_numpy(d), torch.from_numpy(r["depth"]), r["state"], torch.ones(32))
        assert not d_o.any() and not d_d.any() and not cc.any()
        assert not RR.normals(gx, r["state"]).any()
    s64, t64 = RR.truth(c["f64"], o, d, near, 2.0, LEVEL_BOX, n_march=101)
    assert (s64 == 2).all() and np.array_equal(t64, near.astype(np.float64))


def test_first_crossing_special_values():
    """Rule 2 on NaN and +inf: a NaN is outside, +inf inside; the FIRST outside -> inside pair wins; refinements leave states 0 / 2 alone."""
    nan, inf = np.nan, np.inf
    sig = np.array([[0, 0, 2, 0, 2], [0, nan, 2, 2, 2], [nan, 2, 0, 0, 0], [0, 0, 0, inf, 0], [2, 0, 2, 0, 0], [0, 0, 0, 0, nan],
                    [1, 0, 0, 0, 2], [0, 0, 0, 0, 1]], np.float32)
    ta, tb = np.zeros(8, np.float32), np.full(8, 4.0, np.float32)
    a, b, va, vb, st, _ = RR.first_crossing(sig, ta, tb, 1.0)
    assert st.tolist() == [1, 1, 1, 1, 2, 0, 2, 1]
    assert a.tolist() == [1, 1, 0, 2, 0, 0, 0, 3] and b.tolist() == [2, 2, 1, 3, 0, 0, 0, 4]
    assert np.isnan(va[1]) and np.isnan(va[2]) and vb[3] == inf and va[4] == 0 and vb[6] == 0
    sig2 = np.array([[0, 0, 2]] * 8, np.float32)
    sig2[1] = [0, 0, 0]                                        # a state-1 ray without a crossing keeps its bracket
    a2, b2, va2, vb2, st2, lost = RR.first_crossing(sig2, a, b, 1.0, (va, vb, st))
    assert st2.tolist() == st.tolist() and lost.tolist() == [False, True] + [False] * 6
    assert a2.tolist() == [1.5, 1, 0.5, 2.5, 0, 0, 0, 3.5] and b2.tolist() == [2, 2, 1, 3, 0, 0, 0, 4]
    assert np.isnan(va2[1]) and va2[0] == 0 and vb2[0] == 2 and va2[4] == 0 and vb2[5] == 0


def test_implicit_gradient_against_a_central_difference_of_the_truth():
    """Rule 8 in float64 at the truth's hit point against a central difference of the truth depth (64-sample float64 march, 48 bisections)
    under one joint random perturbation of origins, directions and code, on the 128 hit rays of box_rays(128, 64, seed=3, miss=0).
    Step h = 1e-8; EVERY ray within 1e-5 (relative) of its own predicted derivative.

    Both numbers come from a sweep on this oracle (per-ray worst relative error): h = 1e-4, 1e-5, 1e-6, 1e-7 -> 4e-1, 1e-1, 6e-3, 1.6e-3,
    on the few rays whose perturbation crosses a ReLU kink of the wobbling decoder, falling linearly with h; h = 1e-8 -> 3.9e-7 with all
    128 rays clean (median 5e-9); h = 1e-9 -> 7.4e-6 as the float64 resolution of the root starts to show.  1e-5 is 25 times the value at
    the chosen step and 100 times below the first kink error.  The slopes g . d on these rays are 104 .. 257.

    The perturbation is one standard-normal draw per origin, direction and code entry.  A central difference is only as good as the
    function is smooth across [-h, h]: three draws were run while writing this test (generator seeds 11, 12, 13; worst ray 2.8e-4,
    7.8e-7, 5.5e-7).  Under seed 11 the root of ray 9 lies within h |perturbation| of a ReLU kink: its one-sided differences are
    1.4039292 (forward) and 1.4047093 (backward), the forward one agreeing with rule 8's 1.4039293 to 1e-7 -- the formula gives the
    derivative on the side x lies on, the central difference averages the two.  Seed 12 is used; every ray is checked."""
    p64 = {k: v.double() for k, v in planted_params(3, 1, seed=1, wobble=WOBBLE).items()}
    code = _code().double()
    o, d, _ = box_rays(128, 64, seed=3, miss=0.0, dtype=torch.float64)
    g = torch.Generator().manual_seed(12)
    do, dd = torch.randn(128, 3, generator=g, dtype=torch.float64), torch.randn(128, 3, generator=g, dtype=torch.float64)
    dc = torch.randn(1, 256, generator=g, dtype=torch.float64)

    def depth(eps):
        fn = RR.oracle_sigma_fn(p64, code + eps * dc)
        st, t = RR.truth(fn, (o + eps * do).numpy(), (d + eps * dd).numpy(), NEAR, FAR, LEVEL_BOX, n_march=64, n_bisect=48)
        assert (st == 1).all()
        return torch.from_numpy(t)
    t0 = depth(0.0)
    x = (o + t0[:, None] * d).requires_grad_()
    sig = RR.oracle_sigma(p64, x, code)
    assert float((sig.detach() - LEVEL_BOX).abs().max()) < 1e-9
    gx, = torch.autograd.grad(sig.sum(), x)
    _, dsig_dc = torch.autograd.functional.jvp(lambda c_: RR.oracle_sigma(p64, x.detach(), c_), code, dc)
    d_o, d_d, c = RR.implicit_gradient(gx, d, t0, np.ones(128, np.uint8), torch.ones(128, dtype=torch.float64))
    want = (d_o * do).sum(1) + (d_d * dd).sum(1) + c * dsig_dc
    slope = (gx * d).sum(1)
    h = 1e-8
    got = (depth(h) - depth(-h)) / (2 * h)
    rel = ((got - want).abs() / want.abs()).numpy()
    print(f"central difference h={h:g}: worst rel {rel.max():.2e}, median {np.median(rel):.2e}; slopes {float(slope.min()):.0f} .. {float(slope.max()):.0f}")
    assert rel.shape == (128,) and (rel <= 1e-5).all(), (int((rel > 1e-5).sum()), float(rel.max()))


# ------------------------------------------------------------------ the API without a GPU
def test_symbols_and_signatures():
    import supnerf_amd as A
    from supnerf_amd import _lib, geometry as G, ops
    names = ("snr_ray_march_points", "snr_ray_first_crossing", "snr_ray_hit_points")
    assert all(n in _lib.exported_symbols() for n in names)
    lib = _lib.lib()
    assert all(hasattr(lib, n) for n in names)
    assert _lib.header_abi_version() >= 13
    for fn in ("ray_march_points", "ray_first_crossing", "ray_hit_points", "RaySurface"):
        assert hasattr(ops, fn)
    sig = inspect.signature(G.ray_surface)
    assert list(sig.parameters)[:6] == ["model", "rays_o", "rays_d", "near", "far", "shapecode"]
    assert sig.parameters["level"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["level"].default is inspect.Parameter.empty
    assert sig.parameters["n_samples"].default == 64 and len(sig.parameters["refine"].default) == 2
    assert G.RayHits._fields == ("depth", "state", "normal", "width")
    sd = inspect.signature(G.surface_depth)
    assert list(sd.parameters)[:6] == ["model", "cam_pose", "obj_diag", "K", "roi", "shapecode"]
    assert all(sd.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("level", "im_sz", "pixels", "n_samples", "refine", "family"))
    # the C ABI validates before it launches: these return without touching a device
    assert lib.snr_ray_march_points(None, None, None, None, 4, 1, None, None) == -1
    assert lib.snr_ray_march_points(None, None, None, None, 4, 8, None, None) == -1
    assert lib.snr_ray_march_points(None, None, None, None, -1, 8, None, None) == -1
    assert lib.snr_ray_march_points(None, None, None, None, 1 << 40, 8, None, None) == -5
    assert lib.snr_ray_first_crossing(None, 4, 1, 0.0, 1, None, None, None, None, None, None) == -1
    assert lib.snr_ray_first_crossing(None, 4, 8, 0.0, 2, None, None, None, None, None, None) == -1
    assert lib.snr_ray_first_crossing(None, 4, 8, 0.0, 1, None, None, None, None, None, None) == -1
    assert lib.snr_ray_first_crossing(None, 1 << 30, 64, 0.0, 1, None, None, None, None, None, None) == -5
    assert lib.snr_ray_hit_points(None, None, None, None, None, None, None, 4, 0.0, None, None, None, None) == -1
    assert lib.snr_ray_hit_points(None, None, None, None, None, None, None, 0, 0.0, None, None, None, None) == 0


def test_cpu_tensors_and_bad_arguments_raise():
    import supnerf_amd as A
    from supnerf_amd import geometry as G
    model = A.CodeNeRF(shape_blocks=3, texture_blocks=1)
    o, d, sc = torch.zeros(2, 8, 3), torch.ones(2, 8, 3), torch.zeros(2, 256)
    with pytest.raises(A.SnrError):
        G.ray_surface(model, o, d, 0.0, 1.0, sc, level=0.5)                      # CPU tensors: no fallback
    with pytest.raises(A.SnrError):
        G.ray_surface(object(), o, d, 0.0, 1.0, sc, level=0.5)
    with pytest.raises(A.SnrError):
        G.surface_depth(model, torch.eye(4)[:3], 4.0, torch.eye(3), [0, 0, 4, 4], sc[:1], level=0.5)
    with pytest.raises(TypeError):
        G.ray_surface(model, o, d, 0.0, 1.0, sc)                                 # level is required
    with pytest.raises(A.SnrError):
        G.to_decoder_frame(torch.zeros(3, 3), 2.0, family="c")


@pytest.mark.parametrize("family", ["a", "b"])
@pytest.mark.parametrize("flags", [(False, False), (True, False), (False, True), (True, True)])
def test_to_decoder_frame_inverts_to_object_frame(family, flags):
    """Directions: exactly (F is a signed permutation).  Points: exactly for a power-of-two scale; for any other scale (p s) / s rounds
    twice, so within 2 ulp."""
    from supnerf_amd import geometry as G
    v = torch.randn(200, 3, generator=torch.Generator().manual_seed(1))
    kw = dict(family=family, shapenet_obj_cood=flags[0], kitti2nusc=flags[1])
    assert torch.equal(G.to_decoder_frame(G.to_object_frame(v, 4.7, direction=True, **kw), 4.7, direction=True, **kw), v)
    assert torch.equal(G.to_decoder_frame(G.to_object_frame(v, 4.0, **kw), 4.0, **kw), v)
    back = G.to_decoder_frame(G.to_object_frame(v, 4.7, **kw), 4.7, **kw)
    assert float(((back - v).abs() / v.abs()).max()) <= 2 * 2.0 ** -23
    m = torch.tensor(A_frame(*flags)).view(3, 3)
    scale = 4.7 if family == "a" else 4.7 / 2
    assert torch.equal(G.to_decoder_frame(v, 4.7, **kw), (v / scale) @ m.T)
    x = v.clone().requires_grad_()
    G.to_decoder_frame(x, 4.7, **kw).sum().backward()
    assert x.grad is not None and bool(torch.isfinite(x.grad).all())


def A_frame(shapenet_obj_cood, kitti2nusc):
    from supnerf_amd import utils as U
    return U._frame(False, kitti2nusc, shapenet_obj_cood)
