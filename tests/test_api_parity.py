"""The reference-signature API (supnerf_amd.utils / .renderer / .model) on the GPU against the golden vectors
the reference produced, forward and backward.  These read like calls into the reference's own modules."""
import random

import numpy as np
import pytest
import torch

from oracle import supnerf_oracle as O
from oracle_bands import amd, dev, md  # noqa: F401  (amd, dev: fixtures)
from relu_bits import relu_bits_of

pytestmark = pytest.mark.gpu

TOL_RGB, TOL_ACC = 2e-5, 2e-5
TOL_DEPTH_MEAN, TOL_DEPTH_MAX = 1e-5, 1e-4       # metres; north_star bound on the mean is 1e-4
TOL_PSNR_DB = 0.01                               # north_star: PSNR delta <= 0.01 dB


@pytest.fixture(scope="module", params=["fp32", "auto", ("fp32", "auto")], ids=["fp32", "auto", "fp32fwd_bf16x3bwd"])
def model(amd, dev, oracle_params, request):
    """Every API test runs three times: exact fp32 MFMA kernels, 'auto' (= split-bf16 wherever the shape allows it), and the pair
    (exact-fp32 forward, split-bf16 backward on the ReLU bits that forward saved -- where the shape allows it)."""
    m = amd.CodeNeRF(shape_blocks=3, texture_blocks=1)
    m.load_state_dict(oracle_params, strict=True)
    m.precision = request.param
    return m.to(dev)


@pytest.fixture()
def jitter(amd):
    def set_(t):
        amd.utils.JITTER_OVERRIDE = t
    yield set_
    amd.utils.JITTER_OVERRIDE = None


def close_grad(a, b, rel=2e-4):
    b = torch.as_tensor(b).double().cpu()
    return md(a, b) <= rel * float(b.abs().max()) + 1e-7


def check_render(out, g, keys=("rgb", "depth", "acc", "rgb_tgt", "occ")):
    rgb, depth, acc = out[0], out[1], out[2]
    assert md(rgb, g[keys[0]]) < TOL_RGB
    assert float((depth.cpu() - g[keys[1]]).abs().mean()) < TOL_DEPTH_MEAN and md(depth, g[keys[1]]) < TOL_DEPTH_MAX
    assert md(acc, g[keys[2]]) < TOL_ACC
    if len(keys) > 3:
        assert md(out[3], g[keys[3]]) == 0.0 and md(out[4], g[keys[4]]) == 0.0


def psnr(rgb, tgt, occ):
    fg = occ.clone(); fg[occ < 0] = 0
    return float(-10 * torch.log10(((rgb - tgt) ** 2 * fg).sum() / (fg.sum() + 1e-9)))


# ------------------------------------------------------------------ family A (src/utils.py)
@pytest.mark.parametrize("tag", ["a_nusc", "a_demo", "a_kitti"])
def test_render_rays_v2(amd, dev, model, golden, jitter, tag):
    g = golden("render_" + tag)
    jitter(g["jitter"])
    with torch.no_grad():
        out = amd.utils.render_rays_v2(model, dev, g["img"], g["mask_occ"], g["cam_pose"], np.float32(g["obj_diag"]), g["K"], g["roi"],
                                       int(g["n_samples"]), g["shapecode"].to(dev), g["texturecode"].to(dev),
                                       int(g["shapenet_obj_cood"]), 0, kitti2nusc=bool(g["kitti2nusc"]), im_sz=int(g["im_sz"]))
    check_render(out, g)
    # the metric BASELINE.json names: PSNR against the same target, ours vs reference
    p_ref = psnr(g["rgb"], g["rgb_tgt"], g["occ"]); p_our = psnr(out[0].cpu(), g["rgb_tgt"], g["occ"])
    assert abs(p_ref - p_our) < TOL_PSNR_DB


def test_render_rays_v2_pose_on_gpu_no_host_sync(amd, dev, model, golden, jitter):
    """Pose on the device (optimiser mode): near/far are computed there; results agree to fp32 round-off."""
    g = golden("render_a_nusc")
    jitter(g["jitter"])
    with torch.no_grad():
        out = amd.utils.render_rays_v2(model, dev, g["img"], g["mask_occ"], g["cam_pose"].to(dev), np.float32(g["obj_diag"]), g["K"],
                                       g["roi"], 64, g["shapecode"].to(dev), g["texturecode"].to(dev), 1, 0, im_sz=8)
    assert md(out[0], g["rgb"]) < 5e-5 and md(out[1], g["depth"]) < 2e-4 and md(out[2], g["acc"]) < 5e-5


def test_render_rays_v2_flip_and_subset_same_rng_stream(amd, dev, model, golden, jitter):
    """sym_aug coin, ray permutation and jitter come from the same generators in the same order as the reference."""
    g = golden("render_a_flip_subset")
    jitter(g["jitter"])
    seed_flip = next(s for s in range(100) if random.Random(s).uniform(0, 1) > 0.5)
    random.seed(seed_flip); np.random.seed(7)
    with torch.no_grad():
        out = amd.utils.render_rays_v2(model, dev, g["img"], g["mask_occ"], g["cam_pose"], np.float32(g["obj_diag"]), g["K"], g["roi"],
                                       64, g["shapecode"].to(dev), g["texturecode"].to(dev), 1, 1, im_sz=8, n_rays=40)
    check_render(out, g)


def test_jitter_uses_cpu_generator_like_reference(amd, dev, model, golden):
    g = golden("render_a_nusc")
    torch.manual_seed(41)                      # the seed gen_golden.py used for this fixture
    with torch.no_grad():
        out = amd.utils.render_rays_v2(model, dev, g["img"], g["mask_occ"], g["cam_pose"], np.float32(g["obj_diag"]), g["K"], g["roi"],
                                       64, g["shapecode"].to(dev), g["texturecode"].to(dev), 1, 0, im_sz=8)
    check_render(out, g)


def test_render_rays_specified(amd, dev, model, golden, jitter):
    g = golden("render_a_specified")
    jitter(g["jitter"])
    with torch.no_grad():
        out = amd.utils.render_rays_specified(model, dev, g["img"], g["mask_occ"], g["cam_pose"], np.float32(g["obj_diag"]), g["K"],
                                              g["roi"], g["x_vec"].numpy(), g["y_vec"].numpy(), 64, g["shapecode"].to(dev),
                                              g["texturecode"].to(dev), 1, 0)
    # 7 rays x 64 samples: a partially filled 128-point tile
    check_render(out, g)


def test_resize_targets(amd, golden):
    g = golden("resize_targets")
    im, mk = amd.utils._resize(g["img"], g["mask_occ"], 8)
    assert md(im.reshape(-1, 3), g["rgb_tgt"]) == 0 and md(mk.reshape(-1, 1), g["occ"]) == 0


def test_prepare_pixel_samples(amd, dev, golden, jitter):
    g = golden("prepare_pixel_samples")
    for device in ("cpu", dev):
        jitter(g["jitter"])
        np.random.seed(9)
        out = amd.utils.prepare_pixel_samples(g["img"].to(device), g["mask_occ"].to(device), g["cam_pose"].to(device),
                                              np.float32(g["obj_diag"]), g["K"], g["roi"], 20, 64, 1, 0, im_sz=8)
        for a, k in zip(out, ("xyz", "viewdir", "z_vals", "rgb_tgt", "occ")):
            assert md(a, g[k]) < 2e-6, (k, str(device))


def test_render_full_img(amd, dev, model, golden, jitter):
    g = golden("render_full_img")
    jitter(g["jitter"])
    img, depth = amd.utils.render_full_img(model, dev, g["cam_pose"], g["wlh"].numpy(), g["K"], g["roi"], 64, g["shapecode"].to(dev),
                                           g["texturecode"].to(dev), 1, out_depth=True)
    assert md(img, g["img"]) < TOL_RGB and md(depth, g["depth"]) < TOL_DEPTH_MAX


def test_unfused_path_odd_sample_count(amd, dev, model, oracle_params, jitter):
    """n_samples that does not divide 128: encode -> decoder -> composite, three HIP launches, same results."""
    ob = O.synthetic_object(3)
    img, mask = O.synthetic_targets(3, 8)
    S = 48
    jit = torch.rand(S, generator=torch.Generator().manual_seed(3))
    gen = torch.Generator().manual_seed(33)
    sc, tc = torch.randn(1, 256, generator=gen) * 0.3, torch.randn(1, 256, generator=gen) * 0.3
    with torch.no_grad():
        ref = O.render_rays_v2(oracle_params, img, mask, ob["cam_pose"], ob["obj_diag"], ob["K"], ob["roi"], S, sc, tc, True, im_sz=8,
                               jitter=jit)
    jitter(jit)
    with torch.no_grad():
        out = amd.utils.render_rays_v2(model, dev, img, mask, ob["cam_pose"], ob["obj_diag"], ob["K"], ob["roi"], S, sc.to(dev),
                                       tc.to(dev), 1, 0, im_sz=8)
    for a, b, tol in zip(out[:3], ref[:3], (TOL_RGB, TOL_DEPTH_MAX, TOL_ACC)):
        assert md(a, b) < tol


# ------------------------------------------------------------------ family B (src/renderer.py)
@pytest.mark.parametrize("tag", ["b_hit", "b_s32"])
def test_nerf_renderer_render_rays(amd, dev, model, golden, jitter, tag):
    g = golden("render_" + tag)
    jitter(g["jitter"])
    rend = amd.NeRFRenderer(n_samples=int(g["n_samples"]), white_bkgd=True)
    with torch.no_grad():
        out = rend.render_rays(model, dev, g["img"], g["mask_occ"], g["cam_pose"], g["wlh"].numpy(), g["K"], g["roi"],
                               g["shapecode"].to(dev), g["texturecode"].to(dev), im_sz=int(g["im_sz"]))
    check_render(out, g)
    miss = ~g["hit"].bool()
    # rays that miss the box see only the white background and report depth diag/2 * |d| at the collapsed sample
    assert miss.any()


def test_render_rays_v3(amd, dev, model, golden, jitter):
    g, g3 = golden("render_b_hit"), golden("render_v3_b_hit")
    jitter(g3["jitter"])
    with torch.no_grad():
        out = amd.render_rays_v3(model, dev, g["img"], g["mask_occ"], g["cam_pose"], g["wlh"].numpy(), g["K"], g["roi"], 64,
                                 g["shapecode"].to(dev), g["texturecode"].to(dev), 1, 0, im_sz=8, adjust_scale=float(g3["adjust_scale"]))
    assert md(out[0], g3["rgb"]) < 5e-5 and md(out[1], g3["depth"]) < 2e-4 and md(out[2], g3["acc"]) < 5e-5
    with pytest.raises(amd.SnrError):
        amd.render_rays_v3(model, dev, g["img"], g["mask_occ"], g["cam_pose"], g["wlh"].numpy(), g["K"], g["roi"], 32,
                           g["shapecode"].to(dev), g["texturecode"].to(dev), 1, 0, im_sz=8)


# ------------------------------------------------------------------ decoder drop-in (src/model_supnerf.py)
@pytest.mark.parametrize("tag", ["b1_s32", "b3_s64", "b2_s7"])
def test_model_forward(amd, dev, model, golden, tag):
    g = golden("decoder_" + tag)
    with torch.no_grad():
        sig, rgb = model(g["xyz"].to(dev), g["viewdir"].to(dev), g["shapecode"].to(dev), g["texturecode"].to(dev))
    assert sig.shape == g["sigmas"].shape and rgb.shape == g["rgbs"].shape
    assert md(sig, g["sigmas"]) < 2e-5 and md(rgb, g["rgbs"]) < 2e-5


# Gradient tests below are MASK-MATCHED: the oracle differentiates with the ReLU bits the GPU forward saved (tests/relu_bits.py,
# oracle.decoder_forward(relu_masks=...)).  A hidden unit whose pre-activation is within rounding of zero lands on either side of the ReLU
# depending on the summation order, which moves that point's gradient by percents between ANY two correct implementations; rounds 1-2
# therefore accepted 3e-2 ... 1e-1 at small shapes, a band that cannot see a mis-indexed tile.  On the same piecewise-linear function the
# bound is 1e-4 of the gradient's largest entry for both arithmetics.
MASKED_REL = 1e-4


def test_model_forward_backward_vs_oracle_autograd(amd, dev, model, oracle_params):
    gen = torch.Generator().manual_seed(77)
    N, S, B = 8, 16, 2            # 64 points per object: whole wave tiles per object
    xyz = (torch.rand(N, S, 3, generator=gen) - 0.5).requires_grad_()
    vd = torch.randn(N, S, 3, generator=gen); vd = (vd / vd.norm(dim=-1, keepdim=True)).requires_grad_()
    sc = (torch.randn(B, 256, generator=gen) * 0.3).requires_grad_()
    tc = (torch.randn(B, 256, generator=gen) * 0.3).requires_grad_()
    ws, wr = torch.randn(N, S, 1, generator=gen), torch.randn(N, S, 3, generator=gen)
    leaves = [t.detach().to(dev).requires_grad_() for t in (xyz, vd, sc, tc)]
    sig, rgb = model(*leaves)
    masks = relu_bits_of(sig, 3, 1)                       # (before backward: autograd frees what the operator saved)
    ((sig * ws.to(dev)).sum() + (rgb * wr.to(dev)).sum()).backward()
    sig_o, rgb_o = O.decoder_forward(oracle_params, xyz, vd, sc, tc, relu_masks=masks)
    ((sig_o * ws).sum() + (rgb_o * wr).sum()).backward()
    assert md(sig, sig_o) < 2e-5 and md(rgb, rgb_o) < 2e-5
    for a, b, name in zip(leaves, (xyz, vd, sc, tc), ("xyz", "viewdir", "shapecode", "texturecode")):
        assert close_grad(a.grad, b.grad, rel=MASKED_REL), name


@pytest.mark.parametrize("N,S,B", [(10, 7, 2), (3, 5, 3), (1, 33, 1), (6, 16, 2)])
def test_model_backward_ragged_points_per_object(amd, dev, model, oracle_params, N, S, B):
    """Point counts per object that are no multiple of the 32-point wave tile (the reference takes any, src/model_supnerf.py:241-269):
    gradients wrt the codes still come out (the operator pads every object with dummy points), equal to the oracle's autograd."""
    gen = torch.Generator().manual_seed(100 * N + S)
    xyz = (torch.rand(B * N, S, 3, generator=gen) - 0.5).requires_grad_()
    vd = torch.randn(B * N, S, 3, generator=gen); vd = (vd / vd.norm(dim=-1, keepdim=True)).requires_grad_()
    sc = (torch.randn(B, 256, generator=gen) * 0.3).requires_grad_()
    tc = (torch.randn(B, 256, generator=gen) * 0.3).requires_grad_()
    ws, wr = torch.randn(B * N, S, 1, generator=gen), torch.randn(B * N, S, 3, generator=gen)
    leaves = [t.detach().to(dev).requires_grad_() for t in (xyz, vd, sc, tc)]
    sig, rgb = model(*leaves)
    masks = relu_bits_of(sig, 3, 1)
    ((sig * ws.to(dev)).sum() + (rgb * wr.to(dev)).sum()).backward()
    sig_o, rgb_o = O.decoder_forward(oracle_params, xyz, vd, sc, tc, relu_masks=masks)      # (mask-matched, see above)
    ((sig_o * ws).sum() + (rgb_o * wr).sum()).backward()
    assert sig.shape == sig_o.shape and rgb.shape == rgb_o.shape
    assert md(sig, sig_o) < 2e-5 and md(rgb, rgb_o) < 2e-5
    for a, b, name in zip(leaves, (xyz, vd, sc, tc), ("xyz", "viewdir", "shapecode", "texturecode")):
        assert a.grad.shape == b.grad.shape
        assert close_grad(a.grad, b.grad, rel=MASKED_REL), (name, md(a.grad, b.grad), float(b.grad.abs().max()))


@pytest.mark.parametrize("blocks", [(2, 1), (1, 2), (2, 2), (4, 0), (0, 4), (0, 0), (1, 0)])
def test_model_backward_other_block_counts(amd, dev, blocks):
    """Odd and even numbers of 256-wide layers, no shape / no texture blocks: one code instance of the layer serves every chain
    (src/model_codenerf.py:39-63 with other constructor arguments), forward and backward, both arithmetic modes."""
    sb, tb = blocks
    params = O.init_decoder_params(shape_blocks=sb, texture_blocks=tb, seed=11 + 3 * sb + tb, sigma_bias=-2.0)
    gen = torch.Generator().manual_seed(5 + sb * 7 + tb)
    N, S, B = 8, 16, 2
    xyz = (torch.rand(N, S, 3, generator=gen) - 0.5).requires_grad_()
    vd = torch.randn(N, S, 3, generator=gen); vd = (vd / vd.norm(dim=-1, keepdim=True)).requires_grad_()
    sc = (torch.randn(B, 256, generator=gen) * 0.3).requires_grad_()
    tc = (torch.randn(B, 256, generator=gen) * 0.3).requires_grad_()
    ws, wr = torch.randn(N, S, 1, generator=gen), torch.randn(N, S, 3, generator=gen)
    for prec in ("fp32", "bf16x3"):
        m = amd.CodeNeRF(shape_blocks=sb, texture_blocks=tb)
        m.load_state_dict(params, strict=True)
        m = m.to(dev); m.precision = prec
        leaves = [t.detach().to(dev).requires_grad_() for t in (xyz, vd, sc, tc)]
        sig, rgb = m(*leaves)
        masks = relu_bits_of(sig, sb, tb)
        ((sig * ws.to(dev)).sum() + (rgb * wr.to(dev)).sum()).backward()
        for t in (xyz, vd, sc, tc):
            t.grad = None
        sig_o, rgb_o = O.decoder_forward(params, xyz, vd, sc, tc, relu_masks=masks)      # (mask-matched, see above)
        ((sig_o * ws).sum() + (rgb_o * wr).sum()).backward()
        assert md(sig, sig_o) < 2e-5 and md(rgb, rgb_o) < 2e-5, (blocks, prec)
        for a, b, name in zip(leaves, (xyz, vd, sc, tc), ("xyz", "viewdir", "shapecode", "texturecode")):
            if b.grad is None or (name == "shapecode" and sb == 0) or (name == "texturecode" and tb == 0):
                continue
            assert close_grad(a.grad, b.grad, rel=MASKED_REL), (blocks, prec, name, md(a.grad, b.grad), float(b.grad.abs().max()))


# ------------------------------------------------------------------ gradients of the render path
# The two fixtures below hold the REFERENCE's own gradients (8 x 8 rays).  Against them a ReLU flip of one of the 4096 / 2048 points shows
# in the aggregates, so the kernels are held (a) to the mask-matched oracle at 1e-4 (codes) -- the oracle itself is pinned to these very
# fixtures by tests/test_oracle_golden.py -- and (b) to the reference's numbers within FIXTURE_REL, the size of such a flip.
FIXTURE_REL = 2e-3


def test_gradients_family_a(amd, dev, model, golden, jitter, oracle_params):
    g = golden("grads_family_a")
    jitter(g["jitter"])
    sc = g["shapecode"].to(dev).requires_grad_()
    tc = g["texturecode"].to(dev).requires_grad_()
    pose = g["cam_pose"].to(dev).requires_grad_()
    out = amd.utils.render_rays_v2(model, dev, g["img"], g["mask_occ"], pose, np.float32(g["obj_diag"]), g["K"], g["roi"], 64, sc, tc, 1, 0,
                                   im_sz=8)
    masks = relu_bits_of(out[0], 3, 1, n_samples=64)
    loss, l_rgb, l_occ, ps = O.optimise_losses(out[0], out[2], out[3], out[4], 0.1)
    loss.backward()
    assert abs(float(loss.detach()) - float(g["loss"])) < 2e-5 and abs(float(ps.detach()) - float(g["psnr"])) < TOL_PSNR_DB
    assert close_grad(sc.grad, g["d_shapecode"], rel=FIXTURE_REL) and close_grad(tc.grad, g["d_texturecode"], rel=FIXTURE_REL)
    assert close_grad(pose.grad, g["d_cam_pose"], rel=FIXTURE_REL)
    sc_o, tc_o, pose_o = g["shapecode"].clone().requires_grad_(), g["texturecode"].clone().requires_grad_(), g["cam_pose"].clone().requires_grad_()
    with O.given_relu_masks(masks):
        ref = O.render_rays_v2(oracle_params, g["img"], g["mask_occ"], pose_o, np.float32(g["obj_diag"]), g["K"], g["roi"], 64, sc_o, tc_o, True, im_sz=8,
                               jitter=g["jitter"])
        O.optimise_losses(ref[0], ref[2], ref[3], ref[4], 0.1)[0].backward()
    assert close_grad(sc.grad, sc_o.grad, rel=MASKED_REL) and close_grad(tc.grad, tc_o.grad, rel=MASKED_REL)
    assert close_grad(pose.grad, pose_o.grad, rel=5e-4)


def test_gradients_family_b(amd, dev, model, golden, jitter, oracle_params):
    g = golden("grads_family_b")
    jitter(g["jitter"])
    sc = g["shapecode"].to(dev).requires_grad_()
    tc = g["texturecode"].to(dev).requires_grad_()
    pose = g["cam_pose"].to(dev).requires_grad_()
    rend = amd.NeRFRenderer(n_samples=32, white_bkgd=True)
    out = rend.render_rays(model, dev, g["img"], g["mask_occ"], pose, g["wlh"].numpy(), g["K"], g["roi"], sc, tc, im_sz=8)
    masks = relu_bits_of(out[0], 3, 1, n_samples=32)
    loss = O.optimise_losses(out[0], out[2], out[3], out[4], 0.1)[0] + 0.01 * out[1].sum()
    loss.backward()
    assert abs(float(loss) - float(g["loss"])) < 5e-5
    assert close_grad(sc.grad, g["d_shapecode"], rel=FIXTURE_REL) and close_grad(tc.grad, g["d_texturecode"], rel=FIXTURE_REL)
    assert close_grad(pose.grad, g["d_cam_pose"], rel=FIXTURE_REL)
    sc_o, tc_o, pose_o = g["shapecode"].clone().requires_grad_(), g["texturecode"].clone().requires_grad_(), g["cam_pose"].clone().requires_grad_()
    with O.given_relu_masks(masks):
        ref = O.nerf_renderer_render_rays(oracle_params, g["img"], g["mask_occ"], pose_o, g["wlh"].numpy(), g["K"], g["roi"], sc_o, tc_o, n_samples=32,
                                          white_bkgd=True, im_sz=8, jitter=g["jitter"])
        (O.optimise_losses(ref[0], ref[2], ref[3], ref[4], 0.1)[0] + 0.01 * ref[1].sum()).backward()
    assert close_grad(sc.grad, sc_o.grad, rel=MASKED_REL) and close_grad(tc.grad, tc_o.grad, rel=MASKED_REL)
    assert close_grad(pose.grad, pose_o.grad, rel=5e-4)


@pytest.mark.parametrize("S,N", [(4, 24), (8, 24), (16, 24), (32, 24), (128, 24), (4, 7), (16, 3), (8, 1)])
def test_fused_render_gradients_other_sample_counts(amd, dev, model, oracle_params, S, N):
    """The per-ray gradient sums take a different path for every samples-per-ray count that divides 128 (lanes per ray:
    shuffles below 16, one DPP row at 16, row pairs at 32, LDS across waves above): forward and backward against the
    oracle's autograd, family B (per-ray metric depths, white background).  Ray counts that leave a partial 32-point wave tile
    (7 x 4, 3 x 16, 1 x 8 points) are padded with dummy rays inside the operator."""
    ops = amd.ops
    gen = torch.Generator().manual_seed(S + 1000 * (N != 24) * N)
    ro = (torch.randn(N, 3, generator=gen) * 0.05 + torch.tensor([0.0, -2.2, 0.2])).requires_grad_()
    vd = torch.nn.functional.normalize(torch.randn(N, 3, generator=gen) * 0.1 + torch.tensor([0.0, 1.0, 0.0]), dim=-1).requires_grad_()
    t = (torch.sort(torch.rand(N, S, generator=gen), dim=-1)[0] * 1.5 + 1.4).requires_grad_()
    sc = (torch.randn(1, 256, generator=gen) * 0.3).requires_grad_()
    tc = (torch.randn(1, 256, generator=gen) * 0.3).requires_grad_()
    wts = [torch.randn(N, 3, generator=gen), torch.randn(N, generator=gen) * 0.1, torch.randn(N, generator=gen)]
    diag = 5.2
    leaves = [x.detach().to(dev).requires_grad_() for x in (ro, vd, t, sc, tc)]
    cfg = ops.RenderCfg(S, ops.Z_PER_RAY, N, 3, 1, frame=amd.utils._frame(False, False, True), white_bkgd=True, metric_z=True, precision=None)
    out = model.fused_render(leaves[0], leaves[1], leaves[2], torch.ones(1, device=dev), torch.full((1,), diag / 2, device=dev),
                             leaves[3], leaves[4], cfg)
    masks = relu_bits_of(out[0], 3, 1, n_samples=S)
    sum((a * b.to(dev)).sum() for a, b in zip(out, wts)).backward()
    xyz = ro[:, None, :] + vd[:, None, :] * t[:, :, None]
    z_metric = torch.norm(xyz - ro[:, None, :], dim=-1) * (diag / 2)
    xyz_o, vd_o = O.object_frame_transforms(xyz, vd[:, None, :].repeat(1, S, 1), False, False, True)
    sig, rgb = O.decoder_forward(oracle_params, xyz_o, vd_o, sc, tc, relu_masks=masks)      # (mask-matched, see above)
    ref = O.composite(sig, rgb, z_metric, white_bkgd=True)
    sum((a * b).sum() for a, b in zip(ref, wts)).backward()
    assert md(out[0], ref[0]) < TOL_RGB and md(out[1], ref[1]) < TOL_DEPTH_MAX and md(out[2], ref[2]) < TOL_ACC
    # few rays, few samples: nothing averages out, and the depth / direction gradients are differences of large terms -- 5e-4 of the largest
    # entry in fp32 arithmetic on either side; the codes' gradients (sums over all points) are held to the mask-matched 1e-4
    for k, (got, want, rel) in enumerate(zip(leaves, (ro, vd, t, sc, tc), (5e-4, 5e-4, 5e-4, MASKED_REL, MASKED_REL))):
        err, top = (got.grad.cpu() - want.grad).abs(), float(want.grad.abs().max())
        assert close_grad(got.grad, want.grad, rel=rel), (S, k, float(err.max()), top)


def test_training_shapes_volume_rendering_batch(amd, dev, model, golden):
    """Decoder half of ParallelModel.forward (src/trainer_unified_nuscenes.py:120-129): batched codes, per-object z."""
    g = golden("train_step")
    B, n, S = g["xyz"].shape[:3]
    sc = g["shapecode"].to(dev).requires_grad_()
    tc = g["texturecode"].to(dev).requires_grad_()
    sig, rgb = model(g["xyz"].flatten(0, 1).to(dev), g["viewdir"].flatten(0, 1).to(dev), sc, tc)
    out = amd.utils.volume_rendering_batch(sig.view(B, n, S, 1), rgb.view(B, n, S, 3), g["z_vals"].to(dev))
    loss = ((out[0] - g["tgt"].to(dev)) ** 2).mean() + 0.1 * out[2].mean()
    loss.backward()
    assert md(out[0], g["rgb"]) < TOL_RGB and md(out[1], g["depth"]) < TOL_DEPTH_MAX and md(out[2], g["acc"]) < TOL_ACC
    assert abs(float(loss) - float(g["loss"])) < 1e-5
    assert close_grad(sc.grad, g["d_shapecode"]) and close_grad(tc.grad, g["d_texturecode"])


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_training_step_weight_gradients(amd, dev, oracle_params, golden, precision):
    """Training mode (src/trainer_unified_nuscenes.py:120-129,334): loss.backward() also reaches every decoder weight.
    Checked against the reference's own gradients: every bias and small tensor in full, every weight's first row,
    and sum / abs-sum of every tensor.  "fp32": exact fp32 MFMA in the chains and the weight-gradient product;
    "bf16x3": split-bf16 in all three (against the REFERENCE's numbers the comparison cannot be mask-matched; 2048 points here: a hidden unit whose pre-activation sits within round-off of zero flips its ReLU between the two arithmetics and
    moves single entries by up to a percent; the aggregated sums stay at 1e-4)."""
    g = golden("train_step")
    rel = 2e-4 if precision == "fp32" else 5e-3
    rel_sum = 2e-4 if precision == "fp32" else 1e-3
    m = amd.CodeNeRF(shape_blocks=3, texture_blocks=1)
    m.load_state_dict(oracle_params, strict=True)
    m.precision = precision
    m = m.to(dev)
    m.train_decoder_weights = True
    B, n, S = g["xyz"].shape[:3]
    sc = g["shapecode"].to(dev).requires_grad_()
    tc = g["texturecode"].to(dev).requires_grad_()
    sig, rgb = m(g["xyz"].flatten(0, 1).to(dev), g["viewdir"].flatten(0, 1).to(dev), sc, tc)
    out = amd.utils.volume_rendering_batch(sig.view(B, n, S, 1), rgb.view(B, n, S, 3), g["z_vals"].to(dev))
    loss = ((out[0] - g["tgt"].to(dev)) ** 2).mean() + 0.1 * out[2].mean()
    loss.backward()
    assert md(out[0], g["rgb"]) < TOL_RGB and abs(float(loss) - float(g["loss"])) < 1e-5
    assert close_grad(sc.grad, g["d_shapecode"], rel) and close_grad(tc.grad, g["d_texturecode"], rel)
    worst = 0.0
    for name, p in m.named_parameters():
        key = name.replace(".", "_")
        assert p.grad is not None, name
        sums = g["dWsum_" + key].double()
        got = torch.stack([p.grad.double().sum(), p.grad.double().abs().sum()]).cpu()
        assert float((got - sums).abs().max()) <= rel_sum * float(sums[1]) + 1e-7, (name, got, sums)
        for k, a in (("dW_" + key, p.grad), ("dWrow0_" + key, p.grad[0] if p.grad.dim() == 2 else None)):
            if k in g and a is not None:
                worst = max(worst, md(a, g[k]) / (float(g[k].abs().max()) + 1e-30))
                assert close_grad(a, g[k], rel), (name, k, md(a, g[k]), float(g[k].abs().max()))
    print(f"[training gradients vs the reference, {precision}] worst relative entry error {worst:.2e}")


def test_training_step_ragged_points_per_object(amd, dev, oracle_params):
    """Training mode with a point count per object that is no multiple of the 32-point wave tile (2 objects x 5 rays x 7 samples): every
    decoder weight gradient and the code gradients against the oracle's autograd (exact fp32 kernels; the operator pads with dummy
    points that must not contribute to any gradient)."""
    B, n, S = 2, 5, 7
    gen = torch.Generator().manual_seed(41)
    xyz = torch.rand(B * n, S, 3, generator=gen) - 0.5
    vd = torch.randn(B * n, S, 3, generator=gen); vd = vd / vd.norm(dim=-1, keepdim=True)
    sc = (torch.randn(B, 256, generator=gen) * 0.3).requires_grad_()
    tc = (torch.randn(B, 256, generator=gen) * 0.3).requires_grad_()
    ws, wr = torch.randn(B * n, S, 1, generator=gen), torch.randn(B * n, S, 3, generator=gen)
    params = {k: v.clone().requires_grad_() for k, v in oracle_params.items()}
    sig_o, rgb_o = O.decoder_forward(params, xyz, vd, sc, tc)
    ((sig_o * ws).sum() + (rgb_o * wr).sum()).backward()
    m = amd.CodeNeRF(shape_blocks=3, texture_blocks=1)
    m.load_state_dict(oracle_params, strict=True)
    m.precision = "fp32"
    m = m.to(dev)
    m.train_decoder_weights = True
    sc_d, tc_d = sc.detach().to(dev).requires_grad_(), tc.detach().to(dev).requires_grad_()
    sig, rgb = m(xyz.to(dev), vd.to(dev), sc_d, tc_d)
    assert sig.shape == sig_o.shape and md(sig, sig_o) < 2e-5 and md(rgb, rgb_o) < 2e-5
    ((sig * ws.to(dev)).sum() + (rgb * wr.to(dev)).sum()).backward()
    assert close_grad(sc_d.grad, sc.grad) and close_grad(tc_d.grad, tc.grad)
    checked = 0
    for name, p in m.named_parameters():
        ref = params.get(name)
        if ref is None or ref.grad is None:
            continue
        assert p.grad is not None, name
        assert close_grad(p.grad, ref.grad, rel=5e-4), (name, md(p.grad, ref.grad), float(ref.grad.abs().max()))
        checked += 1
    assert checked >= 20, checked


def test_renderer_twins(amd, dev, model, oracle_params, golden, jitter):
    """NeRFRenderer's other methods (src/renderer.py:27-115,169-352) and the small utilities of src/utils.py on the GPU against the
    reference's outputs (fixture `twins`)."""
    g = golden("twins")
    img, mask, pose, K, roi, sc, tc = [g[k] for k in ("img", "mask_occ", "cam_pose", "K", "roi", "shapecode", "texturecode")]
    wlh = g["wlh"].numpy()
    rend = amd.NeRFRenderer(n_samples=32, white_bkgd=True)
    sc_d, tc_d = sc.to(dev), tc.to(dev)
    with torch.no_grad():
        jitter(g["spec_jitter"])
        out = rend.render_rays_specified(model, dev, img, mask, pose, wlh, K, roi, g["spec_x"].numpy(), g["spec_y"].numpy(), sc_d, tc_d)
        check_render(out, g, ("spec_rgb", "spec_depth", "spec_acc", "spec_tgt", "spec_occ"))
        assert md(out[3], g["spec_tgt"]) == 0 and md(out[4], g["spec_occ"]) == 0
        jitter(g["full_jitter"])
        full = rend.render_full_img(model, dev, pose, wlh, K, g["full_roi"], sc_d, tc_d, out_depth=True)
        assert md(full[0], g["full_img"]) < TOL_RGB and md(full[1], g["full_depth"]) < TOL_DEPTH_MAX
        jitter(list(g["virt_b_jitter"]))
        views = rend.render_virtual_imgs(model, dev, wlh, K, sc_d, tc_d, radius=12., pan_num=2, img_sz=12)
        assert md(torch.stack(views), g["virt_b"]) < TOL_RGB
        # family-A turntable: the same two poses through utils.render_full_img (pinned by the render_full_img fixture) == render_virtual_imgs
        jitter(list(g["virt_b_jitter"][:, 0, :]))
        va = amd.utils.render_virtual_imgs(model, dev, wlh, K, 32, sc_d, tc_d, True, radius=12., pan_num=2, img_sz=12)
        want = O.render_virtual_imgs(oracle_params, wlh, K, 32, sc, tc, True, radius=12., pan_num=2, img_sz=12,
                                     jitters=list(g["virt_b_jitter"][:, 0, :]))
        assert md(torch.stack(va), torch.stack(want)) < TOL_RGB
    # GPU twin of prepare_pixel_samples (encode kernel)
    np.random.seed(77)
    jitter(g["pps_jitter"])
    out = rend.prepare_pixel_samples(img.to(dev), mask.to(dev), pose.to(dev), wlh, K, roi, 40, im_sz=8)
    for a, k in zip(out, ("pps_xyz", "pps_viewdir", "pps_z", "pps_tgt", "pps_occ")):
        assert md(a, g[k]) < 5e-6, k
    # the class's small methods and the function-form utilities
    jitter(g["sfr_jitter"])
    assert md(rend.sample_from_ray(g["sfr_rays"].to(dev)), g["sfr_z"]) < 1e-6
    jitter(g["psr_jitter"])
    pxyz, pvd, pz, phit = rend.prepare_sampled_rays(g["util_rays_o"].to(dev), g["util_rays_d"].to(dev), wlh)
    # metric z ~20 m: 5e-6 is 2 ulp
    assert md(pxyz, g["psr_xyz"]) < 2e-6 and md(pz, g["psr_z"]) < 5e-6 and torch.equal(phit.cpu(), g["psr_hit"].bool())
    vr = rend.volume_render(g["vr_sig"].to(dev), g["vr_rgb"].to(dev), g["psr_z"].to(dev))
    assert md(vr[0], g["vr_out_rgb"]) < TOL_RGB and md(vr[1], g["vr_out_depth"]) < TOL_DEPTH_MAX and md(vr[2], g["vr_out_acc"]) < TOL_ACC
    vb = amd.NeRFRenderer(n_samples=32, white_bkgd=False).volume_render_batch(g["vrb_sig"].to(dev), g["vrb_rgb"].to(dev), g["vrb_z"].to(dev))
    assert md(vb[0], g["vrb_out_rgb"]) < TOL_RGB and md(vb[1], g["vrb_out_depth"]) < TOL_DEPTH_MAX and md(vb[2], g["vrb_out_acc"]) < TOL_ACC
    jitter(g["util_jitter"])
    xyz, vdd, z = amd.utils.sample_from_rays(g["util_rays_o"].to(dev), g["util_rays_d"].to(dev), 7.5, 12.25, 9)
    assert md(xyz, g["util_xyz"]) < 2e-6 and md(vdd, g["util_viewdir"]) == 0 and md(z, g["util_z"]) < 1e-6
    xf, _, zf = amd.utils.sample_from_rays(g["util_rays_o"].to(dev), g["util_rays_d"].to(dev), 7.5, 12.25, 9, z_fixed=True)
    assert md(xf, g["util_xyz_fixed"]) < 2e-6 and md(zf, g["util_z_fixed"]) < 1e-6
    leg = amd.utils.volume_rendering(g["legacy_sig"].to(dev), g["legacy_rgb"].to(dev), g["util_z"].to(dev))
    assert md(leg[0], g["legacy_out_rgb"]) < TOL_RGB and md(leg[1], g["legacy_out_depth"]) < TOL_DEPTH_MAX


def test_vis_scene(amd, dev, model, golden):
    """Multi-object scene (scripts/demo.py:425-579) against the picture the reference's building blocks produce."""
    g = golden("scene")
    H, W, S, bs = int(g["H"]), int(g["W"]), int(g["n_samples"]), int(g["ray_batch_size"])
    jit = list(torch.split(g["jitter"], [int(r) for r in g["jitter_rows"]]))
    img, canvas = amd.scene.vis_scene(model, dev, g["obj_poses"], g["obj_wlh"], g["shapecodes"], g["texturecodes"], g["K"], H, W, S,
                                      ray_batch_size=bs, jitters=jit, return_float=True)
    assert md(canvas, g["canvas"]) < TOL_RGB
    assert img.dtype == np.uint8 and img.shape == (H, W, 3)
    assert int(np.abs(img.astype(np.int32) - g["image"].numpy().astype(np.int32)).max()) <= 1      # 255 * 2e-5 can move a pixel across a level
    # another batch size only changes the jitter stream, not the geometry: same covered pixels
    img2 = amd.scene.vis_scene(model, dev, g["obj_poses"], g["obj_wlh"], g["shapecodes"], g["texturecodes"], g["K"], H, W, S, ray_batch_size=257)
    assert np.array_equal((img2 != 255).any(-1) | ~g["valid"].view(H, W).numpy().astype(bool), (img != 255).any(-1) | ~g["valid"].view(H, W).numpy().astype(bool))


# ------------------------------------------------------------------ batched objects, full size properties
def test_batched_objects_equal_single_objects(amd, dev, model):
    """C3 shape in miniature: B objects in one launch == B single-object launches (object-major codes, per-object z)."""
    ops = amd.ops
    B, N, S = 3, 64, 64
    gen = torch.Generator().manual_seed(5)
    ro = (torch.randn(B * N, 3, generator=gen) * 0.2 + torch.tensor([0., -11., 1.])).to(dev)
    vd = torch.randn(B * N, 3, generator=gen) * 0.1 + torch.tensor([0., 1., 0.]); vd = (vd / vd.norm(dim=-1, keepdim=True)).to(dev)
    z = torch.sort(torch.rand(B, S, generator=gen) * 5 + 8.5, dim=-1)[0].to(dev)
    sc, tc = (torch.randn(B, 256, generator=gen) * 0.3).to(dev), (torch.randn(B, 256, generator=gen) * 0.3).to(dev)
    div = torch.tensor([5.1, 5.6, 4.9], device=dev)
    with torch.no_grad():
        cfg = ops.RenderCfg(S, ops.Z_PER_OBJECT, N, 3, 1, precision=None)     # None: the fixture's model.precision decides (fp32 | auto)
        full = model.fused_render(ro, vd, z, div, None, sc, tc, cfg)
        for b in range(B):
            cfg1 = ops.RenderCfg(S, ops.Z_SHARED, N, 3, 1, precision=None)
            one = model.fused_render(ro[b * N:(b + 1) * N], vd[b * N:(b + 1) * N], z[b], div[b:b + 1], None, sc[b:b + 1], tc[b:b + 1], cfg1)
            for a, c in zip(full, one):
                assert torch.equal(a[b * N:(b + 1) * N], c)


def test_full_size_properties(amd, dev, model):
    """BASELINE config 2 size (4096 rays x 64 samples): size-independent properties instead of an oracle run --
    determinism, independence of rays (any subset renders to the same values), opacity bounds."""
    ops = amd.ops
    N, S = 4096, 64
    gen = torch.Generator().manual_seed(9)
    ro = (torch.randn(N, 3, generator=gen) * 0.3 + torch.tensor([0., -12., 1.])).to(dev)
    vd = torch.randn(N, 3, generator=gen) * 0.15 + torch.tensor([0., 1., 0.]); vd = (vd / vd.norm(dim=-1, keepdim=True)).to(dev)
    z = torch.linspace(9.3, 14.7, S).to(dev)
    sc, tc = (torch.randn(1, 256, generator=gen) * 0.3).to(dev), (torch.randn(1, 256, generator=gen) * 0.3).to(dev)
    div = torch.tensor([5.4], device=dev)
    cfg = ops.RenderCfg(S, ops.Z_SHARED, N, 3, 1, precision=None)
    with torch.no_grad():
        a = model.fused_render(ro, vd, z, div, None, sc, tc, cfg)
        b = model.fused_render(ro, vd, z, div, None, sc, tc, cfg)
        idx = torch.randperm(N, generator=gen)[:1000].to(dev)
        cfg_s = ops.RenderCfg(S, ops.Z_SHARED, 1000, 3, 1, precision=None)
        sub = model.fused_render(ro[idx], vd[idx], z, div, None, sc, tc, cfg_s)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for x, y in zip(a, sub):
        assert torch.equal(x[idx], y)
    assert bool((a[2] >= 0).all()) and bool((a[2] <= 1 + 1e-6).all())
    assert bool((a[1] >= 0).all()) and bool((a[1] <= float(z[-1]) + 1e-3).all())
