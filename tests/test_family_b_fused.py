"""Family B (``NeRFRenderer.render_rays``, src/renderer.py:91-166: per-ray box bounds + per-ray stratified depths) as ONE launch
(``SNR_Z_BOX``), against the CPU oracle -- which the reference's own family-B vectors pin (``render_b_*``, ``grads_family_b``,
``twins`` fixtures; tests/test_oracle_golden.py).

* the kernel prologue (slab test, hit / miss bounds, depth table, points, metric z, hit map) against the oracle's ``aabb_sampled_rays``;
* the in-kernel jitter is the number ``torch.rand_like`` would have drawn, and the device generator advances like that call;
* forward + gradients wrt codes and pose (THROUGH the box bounds) against the oracle's autograd at every lanes-per-ray path
  (S = 4 ... 128), with bounds detached (``render_rays_v3``), with padded ragged ray counts;
* BASELINE's shape, 4096 rays x 64 samples with a hit / miss mix and a white background, both arithmetics (north_star names
  ``render_rays`` in src/renderer.py first, and 4096 x 64 is that method's default).
"""
import numpy as np
import pytest
import torch

from oracle import supnerf_oracle as O
from oracle_bands import amd, check_per_ray, dev, make_model, md, per_ray_errors, rel  # noqa: F401  (amd, dev: fixtures)

pytestmark = pytest.mark.gpu

TOL_RGB, TOL_ACC, TOL_DEPTH_MEAN, TOL_DEPTH_MAX, TOL_PSNR = 2e-5, 2e-5, 1e-5, 1e-4, 0.01


def scene(index, im_sz, S, seed):
    """One synthetic car whose roi is wider than the box, so the pixel grid holds hits AND misses."""
    ob = O.synthetic_object(index)
    img, mask = O.synthetic_targets(index, im_sz)
    g = torch.Generator().manual_seed(seed)
    sc, tc = torch.randn(1, 256, generator=g) * 0.3, torch.randn(1, 256, generator=g) * 0.3
    jit = torch.rand(im_sz * im_sz, S, generator=g)
    return ob, img, mask, sc, tc, jit


# ------------------------------------------------------------------ prologue alone
@pytest.mark.parametrize("S", [64, 32, 8])
def test_box_prologue_matches_oracle(amd, dev, S):
    ob, img, mask, _, _, jit = scene(7, 24, S, 1)
    rays_o, viewdir = O.pixel_rays(ob["K"], ob["cam_pose"], ob["roi"], uv_steps=[24, 24])
    xyz, vd, z_vals, hit = O.aabb_sampled_rays(rays_o, viewdir, ob["wlh"], S, jit)
    assert bool(hit.any()) and bool((~hit).any())
    rend = amd.NeRFRenderer(n_samples=S)
    amd.utils.JITTER_OVERRIDE = jit
    try:
        out = rend.prepare_sampled_rays(rays_o.to(dev), viewdir.to(dev), ob["wlh"])
    finally:
        amd.utils.JITTER_OVERRIDE = None
    assert torch.equal(out[3].cpu(), hit)
    assert md(out[0], xyz) == 0.0 and md(out[1], vd) == 0.0 and md(out[2], z_vals) == 0.0       # bit for bit the reference's fp32 arithmetic


def test_kernel_jitter_is_torch_rand_like(amd, dev):
    """No jitter tensor: the kernel regenerates torch.rand_like's numbers from the generator state and the generator moves on as if
    rand_like had run -- for a table small enough for one Philox call per thread and for one that takes several rounds."""
    ob = O.synthetic_object(7)
    rend = amd.NeRFRenderer(n_samples=64)
    for im_sz in (24, 160):                  # 36 864 and 1 638 400 samples (the second: several elements per generator thread)
        rays_o, viewdir = O.pixel_rays(ob["K"], ob["cam_pose"], ob["roi"], uv_steps=[im_sz, im_sz])
        rays_o, viewdir = rays_o.to(dev), viewdir.to(dev)
        torch.manual_seed(1234)
        junk = torch.rand(1000, device=dev)                                  # (a non-zero generator offset)
        jit = torch.rand_like(torch.empty(rays_o.shape[0], 64, device=dev))
        after = torch.rand(8, device=dev)
        amd.utils.JITTER_OVERRIDE = jit
        try:
            want = rend.prepare_sampled_rays(rays_o, viewdir, ob["wlh"])
        finally:
            amd.utils.JITTER_OVERRIDE = None
        torch.manual_seed(1234)
        junk2 = torch.rand(1000, device=dev)
        got = rend.prepare_sampled_rays(rays_o, viewdir, ob["wlh"])
        after2 = torch.rand(8, device=dev)
        assert torch.equal(junk, junk2)
        assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2]), im_sz
        assert torch.equal(after, after2), "the generator did not advance like torch.rand_like"


# ------------------------------------------------------------------ render + gradients, small
def oracle_b(params, ob, img, mask, sc0, tc0, jit, S, im_sz, white=True, depth_w=0.01, dtype=torch.float32):
    """The oracle's family-B render + loss + autograd; ``dtype=torch.float64`` gives the same computation in double precision."""
    c = lambda t: t.to(dtype)
    params = {k: c(v) for k, v in params.items()}
    img, mask, jit = c(img), c(mask), c(jit)
    sc, tc, pose = c(sc0).clone().requires_grad_(), c(tc0).clone().requires_grad_(), c(ob["cam_pose"]).clone().requires_grad_()
    out = O.nerf_renderer_render_rays(params, img, mask, pose, ob["wlh"], c(ob["K"]), ob["roi"], sc, tc, n_samples=S, white_bkgd=white,
                                      im_sz=im_sz, jitter=jit)
    loss = O.optimise_losses(out[0], out[2], out[3], out[4], 0.1)[0] + depth_w * out[1].mean()
    loss.backward()
    return [t.detach() for t in out], float(loss), sc.grad.clone(), tc.grad.clone(), pose.grad.clone()


def hip_b(amd, dev, model, ob, img, mask, sc0, tc0, jit, S, im_sz, white=True, depth_w=0.01):
    sc, tc = sc0.to(dev).requires_grad_(), tc0.to(dev).requires_grad_()
    pose = ob["cam_pose"].to(dev).requires_grad_()
    rend = amd.NeRFRenderer(n_samples=S, white_bkgd=white)
    amd.utils.JITTER_OVERRIDE = jit
    try:
        out = rend.render_rays(model, dev, img, mask, pose, ob["wlh"], ob["K"], ob["roi"], sc, tc, im_sz=im_sz)
    finally:
        amd.utils.JITTER_OVERRIDE = None
    loss = O.optimise_losses(out[0], out[2], out[3], out[4], 0.1)[0] + depth_w * out[1].mean()
    loss.backward()
    return out, float(loss), sc.grad, tc.grad, pose.grad


@pytest.mark.parametrize("S,im_sz", [(64, 16), (128, 12), (32, 16), (16, 16), (8, 16), (4, 16), (64, 5), (16, 7)])
def test_box_render_and_gradients_small(amd, dev, oracle_params, S, im_sz):
    """Every lanes-per-ray path of the backward tail (S = 4 ... 128) and ray counts that need padding (5 x 5, 7 x 7), exact fp32 kernels:
    the gradient wrt the pose includes the path through z_in / z_out (src/renderer.py:102-108)."""
    ob, img, mask, sc0, tc0, jit = scene(11, im_sz, S, 5)
    ref, loss_ref, g_sc, g_tc, g_pose = oracle_b(oracle_params, ob, img, mask, sc0, tc0, jit, S, im_sz)
    model = make_model(amd, dev, oracle_params, "fp32")
    out, loss, d_sc, d_tc, d_pose = hip_b(amd, dev, model, ob, img, mask, sc0, tc0, jit, S, im_sz)
    assert md(out[0], ref[0]) < TOL_RGB and md(out[2], ref[2]) < TOL_ACC and md(out[1], ref[1]) < TOL_DEPTH_MAX
    assert abs(loss - loss_ref) < 5e-6
    # Gradient bound DERIVED per case, not fitted: the same computation on the oracle in float64 tells how far an fp32 evaluation of this
    # gradient sits from the true value (the pose gradient at few samples per ray is a small difference of large terms: the fp32 oracle
    # itself is 5e-4 / 9e-4 off at S = 8 / 4).  That distance is ONE sample of the rounding noise of this gradient (a few grazing rays, whose
    # bounds move by (hb - o) / d^2 per unit of direction, carry most of it); the fp32 kernels, another sample of it, may sit at most four
    # times as far from the float64 value, plus 1e-4.
    _, _, t_sc, t_tc, t_pose = oracle_b(oracle_params, ob, img, mask, sc0, tc0, jit, S, im_sz, dtype=torch.float64)
    for name, got, ref32, true in (("sc", d_sc, g_sc, t_sc), ("tc", d_tc, g_tc, t_tc), ("pose", d_pose, g_pose, t_pose)):
        floor = rel(ref32, true)
        assert rel(got, true) < 4 * floor + 1e-4, (name, rel(got, true), floor)


def test_box_bounds_gradient_matters_and_detach(amd, dev, oracle_params):
    """(a) the pose gradient THROUGH the bounds is not negligible (so the test above would see it missing); (b) with the bounds detached
    (render_rays_v3: numpy slab test, src/renderer.py:425-432) the kernel matches the oracle's detached gradient."""
    S, im_sz = 64, 12
    ob, img, mask, sc0, tc0, jit = scene(11, im_sz, S, 5)
    model = make_model(amd, dev, oracle_params, "fp32")
    res = {}
    for detach in (False, True):
        pose = ob["cam_pose"].clone().requires_grad_()
        rays_o, viewdir = O.pixel_rays(ob["K"], pose, ob["roi"], uv_steps=[im_sz, im_sz])
        xyz, vd, z_vals, _ = O.aabb_sampled_rays(rays_o, viewdir, ob["wlh"], S, jit, detach_bounds=detach)
        sig, rgb = O.decoder_forward(oracle_params, xyz, vd, sc0, tc0)
        o = O.composite(sig, rgb, z_vals, white_bkgd=True)
        (o[0].sum() + 0.1 * o[1].sum() + o[2].sum()).backward()
        pose_d = ob["cam_pose"].to(dev).requires_grad_()
        ro, vdd = amd.utils.get_rays(ob["K"], pose_d, ob["roi"], uv_steps=[im_sz, im_sz])
        rend = amd.NeRFRenderer(n_samples=S, white_bkgd=True)
        h = rend._render(model, dev, ro, vdd, ob["wlh"], sc0.to(dev), tc0.to(dev), False, True, jitter=jit, detach_bounds=detach)
        (h[0].sum() + 0.1 * h[1].sum() + h[2].sum()).backward()
        assert md(h[0], o[0]) < TOL_RGB
        # bound derived like above: the same gradient on the oracle in float64
        p64 = ob["cam_pose"].double().clone().requires_grad_()
        ro64, vd64 = O.pixel_rays(ob["K"].double(), p64, ob["roi"], uv_steps=[im_sz, im_sz])
        x64, v64, z64, _ = O.aabb_sampled_rays(ro64, vd64, ob["wlh"], S, jit.double(), detach_bounds=detach)
        s64, r64 = O.decoder_forward({k: v.double() for k, v in oracle_params.items()}, x64, v64, sc0.double(), tc0.double())
        o64 = O.composite(s64, r64, z64, white_bkgd=True)
        (o64[0].sum() + 0.1 * o64[1].sum() + o64[2].sum()).backward()
        floor = rel(pose.grad, p64.grad)
        assert rel(pose_d.grad, p64.grad) < 4 * floor + 1e-4, (detach, rel(pose_d.grad, p64.grad), floor)
        res[detach] = pose.grad.clone()
    assert rel(res[False], res[True]) > 1e-2


# ------------------------------------------------------------------ BASELINE's shape
@pytest.fixture(scope="module")
def full_oracle(oracle_params):
    """4096 x 64, family B, on the CPU oracle (forward + backward to codes and pose): once for both arithmetics."""
    S, im_sz = 64, 64
    ob, img, mask, sc0, tc0, jit = scene(100, im_sz, S, 100)
    ref = oracle_b(oracle_params, ob, img, mask, sc0, tc0, jit, S, im_sz)
    true = oracle_b(oracle_params, ob, img, mask, sc0, tc0, jit, S, im_sz, dtype=torch.float64)
    rays_o, viewdir = O.pixel_rays(ob["K"], ob["cam_pose"], ob["roi"], uv_steps=[im_sz, im_sz])
    hit = O.aabb_sampled_rays(rays_o, viewdir, ob["wlh"], S, jit)[3]
    return dict(ob=ob, img=img, mask=mask, sc0=sc0, tc0=tc0, jit=jit, ref=ref, true=true, hit=hit)


@pytest.mark.parametrize("precision", ["fp32", "auto"])
def test_family_b_full_size_against_oracle(amd, dev, oracle_params, full_oracle, precision):
    r = full_oracle
    ref, loss_ref, g_sc, g_tc, g_pose = r["ref"]
    n_hit = int(r["hit"].sum())
    assert 400 < n_hit < 3700, n_hit                  # a real hit / miss mix
    model = make_model(amd, dev, oracle_params, precision)
    if precision == "auto":
        assert amd.ops.resolve_precision(model.precision, 3, 1, 4096 * 64) == amd.ops.BF16X3
    out, loss, d_sc, d_tc, d_pose = hip_b(amd, dev, model, r["ob"], r["img"], r["mask"], r["sc0"], r["tc0"], r["jit"], 64, 64)
    assert out[0].shape == (4096, 3)
    # (a ray that misses the box is NOT white: its 64 samples collapse onto the point o_n - d, whose last sample has delta 1e10 and takes
    # the whole weight, src/renderer.py:50-56 -- the oracle does the same, the comparison below covers those rays)
    assert md(out[0], ref[0]) < TOL_RGB and md(out[2], ref[2]) < TOL_ACC
    assert float((out[1].detach().cpu() - ref[1]).abs().mean()) < TOL_DEPTH_MEAN and md(out[1], ref[1]) < TOL_DEPTH_MAX
    psnr = lambda rgb: float(-10 * torch.log10(((rgb - ref[3]) ** 2).mean()))
    assert abs(psnr(out[0].detach().cpu()) - psnr(ref[0])) < TOL_PSNR
    assert abs(loss - loss_ref) < 2e-6
    e = dict(sc=rel(d_sc, g_sc), tc=rel(d_tc, g_tc), pose=rel(d_pose, g_pose))
    t_pose = r["true"][4]
    floor, e_true = rel(g_pose, t_pose), rel(d_pose, t_pose)
    print(f"[family B 4096x64, {precision}] {n_hit} hits; rgb {md(out[0], ref[0]):.2e} depth mean "
          f"{float((out[1].detach().cpu() - ref[1]).abs().mean()):.2e} grad rel err codes {e['sc']:.2e}/{e['tc']:.2e} pose {e['pose']:.2e} "
          f"(pose vs the float64 oracle: kernels {e_true:.2e}, the fp32 oracle itself {floor:.2e})")
    assert max(e["sc"], e["tc"]) < 2e-4, e
    # the pose gradient of THIS loss is ill-conditioned in fp32 whoever computes it: the reference's own fp32 evaluation (the oracle) is
    # 5.5e-3 away from the float64 value here (grazing rays: d t_near / d direction ~ (hb - o) / d^2).  Bound derived from that, see
    # test_box_render_and_gradients_small; the per-ray test below is the discriminating one.
    assert e_true < 4 * floor + 1e-4, (e_true, floor)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_family_b_per_ray_gradients_mask_matched(amd, dev, oracle_params, precision):
    """The gradient wrt every ray's origin and direction (INCLUDING the path through that ray's box bounds) and wrt the latent terms
    against the oracle's autograd, ray by ray at 1024 rays x 64 samples, on the SAME piecewise-linear function: the oracle's ReLU
    derivatives are the bits the forward launch saved (tests/relu_bits.py).  Without that, a hidden unit whose pre-activation is within
    rounding of zero flips between two correct implementations and moves its ray by percents (6 of 1024 rays in split-bf16), which
    forces a band wide enough to hide an indexing slip.  With it every ray is held to 1e-3 of ITS OWN float64 gradient (or to 8x what
    the fp32 oracle manages on that very ray: grazing rays are ill-conditioned in fp32 whoever computes them)."""
    from relu_bits import decode_relu_bits
    from supnerf_amd import renderer as R
    ops = amd.ops
    S, im_sz = 64, 32
    ob, img, mask, sc0, tc0, jit = scene(100, im_sz, S, 9)
    ro, vd = O.pixel_rays(ob["K"], ob["cam_pose"], ob["roi"], uv_steps=[im_sz, im_sz])
    N = ro.shape[0]
    g = torch.Generator().manual_seed(2)
    w_rgb, w_d, w_a = torch.rand(N, 3, generator=g), torch.rand(N, generator=g) * 0.1, torch.rand(N, generator=g)

    model = make_model(amd, dev, oracle_params, precision)
    with torch.no_grad():
        lat = model.latent_terms(sc0.to(dev), tc0.to(dev))
    _, half, zs = R._box_constants(ob["wlh"], 1, dev)
    cfg = ops.RenderCfg(S, ops.Z_BOX, N, 3, 1, white_bkgd=True, metric_z=True, precision=precision, box_half=half)
    args = (ro.to(dev), vd.to(dev), jit.to(dev), None, zs, lat, model.packed_weights(), cfg)
    fw = ops.render_fwd(*args, save_for_bwd=True)
    d_o, d_d, _, d_lat = ops.render_bwd(*args, fw[3], fw[4], fw[5], w_rgb.to(dev), w_d.to(dev), w_a.to(dev))
    masks = decode_relu_bits(fw[5], N * S, 3, 1)

    def oracle(dtype):
        c = lambda t: t.to(dtype)
        o, d = c(ro).clone().requires_grad_(), c(vd).clone().requires_grad_()
        sc, tc = c(sc0).clone().requires_grad_(), c(tc0).clone().requires_grad_()
        xyz, v, z, hit = O.aabb_sampled_rays(o, d, ob["wlh"], S, c(jit))
        sig, rgb = O.decoder_forward({k: c(t) for k, t in oracle_params.items()}, xyz, v, sc, tc, relu_masks=masks)
        out = O.composite(sig, rgb, z, white_bkgd=True)
        ((out[0] * c(w_rgb)).sum() + (out[1] * c(w_d)).sum() + (out[2] * c(w_a)).sum()).backward()
        return o.grad, d.grad, hit, [t.detach() for t in out], sc.grad, tc.grad
    go32, gd32, hit, out32, _, _ = oracle(torch.float32)
    go64, gd64, _, _, gsc64, gtc64 = oracle(torch.float64)
    assert bool(hit.any()) and bool((~hit).any())
    assert md(fw[0], out32[0]) < TOL_RGB and md(fw[1], out32[1]) < TOL_DEPTH_MAX and md(fw[2], out32[2]) < TOL_ACC
    bad = []
    for name, got, ref32, true in (("d_rays_o", d_o, go32, go64), ("d_rays_d", d_d, gd32, gd64)):
        bad += check_per_ray(f"{name}, {precision}", got, ref32, true)
        err, floor = per_ray_errors(got, ref32, true)
        assert float(err.median()) < 2e-5 + 4 * float(floor.median()), (name, float(err.median()), float(floor.median()))
    assert not bad, bad
    # the codes' gradients through the latent terms (the kernel's d_latent chained through the latent layers by torch): tight once the masks agree
    sc, tc = sc0.to(dev).requires_grad_(), tc0.to(dev).requires_grad_()
    model.latent_terms(sc, tc).backward(d_lat)
    e_sc, e_tc = rel(sc.grad, gsc64), rel(tc.grad, gtc64)
    print(f"[mask-matched code gradients, {precision}] {e_sc:.1e} / {e_tc:.1e}")
    assert max(e_sc, e_tc) < (2e-5 if precision == "fp32" else 1e-4)
