"""Per-object latent gradients across the edges of the backward's three steps, against the float64 oracle, mask-matched.

Every backward launch with code gradients (1) writes one row of latent-gradient partials per wave tile, (2) sums them per object in a
deterministic tree (``snr_launch_reduce_latent_``, csrc/snr_aux.hip: chunks of RED_CHUNK = 32 tiles, one grid row per object, ping-pong
scratch) and (3) does both in one workspace sized by ``snr_decoder_bwd_ws_bytes`` (csrc/snr_decoder.hip) for 32-point tiles, whose tree scratch starts
right behind the partials of the kernel that ran.  Every comparison here is per object: each object's (NLAT, 256) latent gradient and its
code-gradient rows against that object's own float64 values, scaled by that object's own max, with distinct codes and distinct upstream
weights per object -- so a row that went to a neighbour, or a tile counted twice, cannot hide behind a larger object.

Which kernel a parametrisation reaches (a change to these predicates moves the coverage below):
* "bf16x3" (and the backward of the pair ("fp32", "bf16x3")): ``bf16_bwd16_kernel`` (csrc/snr_bf16.hip) whenever ``snr_bf16_supported_``
  holds: shape_blocks + texture_blocks <= 4 and points per object % 32 == 0.  Tile: 32 points.
* "fp32": ``decoder_backward`` (csrc/snr_decoder.hip) takes the two-wave ``decoder_bwd16_kernel`` (csrc/snr_mlp16_bwd.hip, 64-point tiles)
  when ``snr_fp32_bwd16_supported_`` holds: no training dumps, points per object % 64 == 0 and, in render mode, S <= 64 with 64 % S == 0;
  otherwise the round-2 ``decoder_bwd_kernel`` (32-point tiles).  So in the points decoder 32, 96, 160, 32*31, 32*33, 32*1025 and the
  ragged 70 (padded to 96) are round-2 objects, and 64, 128, 32*32, 64*31..64*33, 32*1024 and the ragged 33 and 100 (padded to 64 and
  128) are two-wave; in the render, S = 128 is always round-2.
* Tree depth: an object of T tiles takes ceil(log32 T) levels -- 31/32 tiles one level, 33 two, 1024 two, 1025 three.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import planted_decoder as PD
from oracle import supnerf_oracle as O
from oracle_bands import amd, band_of, capture_latent, check_per_object, check_per_ray, dev, make_model  # noqa: F401  (amd, dev: fixtures)
from relu_bits import decode_relu_bits, relu_bits_of

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "bf16x3", ("fp32", "bf16x3")]
PREC_ID = lambda p: "-".join(p) if isinstance(p, tuple) else p


def codes(B, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, 256, generator=g) * 0.3 for _ in range(2)]


def obj_scale(B, per_obj, seed):
    """A distinct factor per object (over three decades), repeated over its points."""
    g = torch.Generator().manual_seed(seed)
    s = 10.0 ** (torch.rand(B, generator=g) * 3 - 1.5)
    return s.repeat_interleave(per_obj)


# ------------------------------------------------------------------ a. points decoder (snr_decoder_bwd, mode 0)
def oracle_latent(p, dt, lat, codes, lat_on):
    """The oracle's latent terms in dtype ``dt``, their gradient kept: ``lat`` as given, or those of ``codes`` (sc, tc) whose ReLU
    derivative is ``lat_on`` (the GPU's z > 0: a pre-activation within rounding of zero must not flip between the two sides of the
    comparison either).  Returns (latent, sc, tc), the codes None when ``lat`` is given."""
    if codes is None:
        return lat.to(dt).clone().requires_grad_(), None, None
    sc, tc = [c.to(dt).clone().requires_grad_() for c in codes]
    lat = O.latent_terms(p, sc, tc, relu_mask=lat_on)
    lat.retain_grad()
    return lat, sc, tc


def grad_of(x):
    return None if x is None else x.grad


def oracle_points(params, xyz, vd, masks, ws, wr, dt, lat=None, codes=None, lat_on=None):
    """Gradients of sum(sig ws) + sum(rgb wr), xyz (P,3) object-major, latent terms as ``oracle_latent`` makes them: (d_latent,
    d_shapecode, d_texturecode)."""
    p = {k: v.to(dt) for k, v in params.items()}
    lat, sc, tc = oracle_latent(p, dt, lat, codes, lat_on)
    s, r = O.decoder_forward(p, xyz.to(dt)[:, None], vd.to(dt)[:, None], None, None, relu_masks=masks, latent=lat)
    ((s.reshape(-1) * ws.to(dt)).sum() + (r.reshape(-1, 3) * wr.to(dt)).sum()).backward()
    return lat.grad, grad_of(sc), grad_of(tc)


def run_points(amd, dev, B, n, precision, blocks=(3, 1), seed=0):
    sb, tb = blocks
    params = O.init_decoder_params(sb, tb, seed=seed, sigma_bias=-2.0)
    P = B * n
    g = torch.Generator().manual_seed(1000 + n + 7 * B)
    xyz = torch.rand(P, 3, generator=g) * 2 - 1
    vd = F.normalize(torch.randn(P, 3, generator=g), dim=-1)
    sc, tc = codes(B, n + B)
    sc[:, 0] += torch.arange(B) * 0.01                      # (distinct codes even where the generator is reused)
    s = obj_scale(B, n, n * 31 + B)
    ws = torch.randn(P, generator=g) * s
    wr = torch.randn(P, 3, generator=g) * s[:, None]
    m = make_model(amd, dev, params, precision, blocks)
    lats = capture_latent(m)
    sc_d, tc_d = sc.to(dev).requires_grad_(), tc.to(dev).requires_grad_()
    sig, rgb = m(xyz.to(dev), vd.to(dev), sc_d, tc_d)                # the public path: ops.DecoderPoints (pads ragged objects)
    masks = relu_bits_of(sig, sb, tb)
    ((sig.reshape(-1) * ws.to(dev)).sum() + (rgb.reshape(-1, 3) * wr.to(dev)).sum()).backward()
    lat = lats[0]
    on = (lat.detach() > 0).cpu()
    ref = {dt: oracle_points(params, xyz, vd, masks, ws, wr, dt, codes=(sc, tc), lat_on=on) for dt in (torch.float32, torch.float64)}
    pairs = [("d_latent", lat.grad, ref[torch.float32][0], ref[torch.float64][0])]
    if sb:
        pairs.append(("d_shapecode", sc_d.grad, ref[torch.float32][1], ref[torch.float64][1]))
    if tb:
        pairs.append(("d_texturecode", tc_d.grad, ref[torch.float32][2], ref[torch.float64][2]))
    check_per_object(pairs, band_of(precision))


# points per object: (n, objects) -- fp32 kernel for each n in the module docstring; bf16x3 is 32-point tiles throughout
SMALL = [32, 64, 96, 128, 160]                    # below, at and straddling a 128-point workgroup; 32, 96, 160: round-2 fp32
EDGE32 = [32 * 31, 32 * 32, 32 * 33]              # 31 / 32 / 33 tiles of 32 points: one level, one level, two levels
EDGE64 = [64 * 31, 64 * 32, 64 * 33]              # the same boundary for the two-wave fp32 kernel's 64-point tiles (62..66 tiles of 32)
DEEP = [32 * 1024, 32 * 1025]                     # 1024 tiles: two levels; 1025: three (fp32: 32*1024 two-wave, 512 tiles, two levels)
POINT_CASES = [(n, B) for n in SMALL for B in (1, 3, 64)] + [(n, B) for n in EDGE32 + EDGE64 for B in (1, 3)] + [(n, 1) for n in DEEP]


@pytest.mark.parametrize("precision", PRECISIONS, ids=PREC_ID)
@pytest.mark.parametrize("n,B", POINT_CASES, ids=lambda v: str(v))
def test_points_latent_gradient_per_object(amd, dev, n, B, precision):
    run_points(amd, dev, B, n, precision)


@pytest.mark.parametrize("precision", PRECISIONS, ids=PREC_ID)
@pytest.mark.parametrize("n", [33, 70, 100])
def test_points_ragged_objects(amd, dev, n, precision):
    """Ragged counts through ops.DecoderPoints, padded per object to 64 / 96 / 128 points (fp32: two-wave / round-2 / two-wave); the
    dummy points must add nothing to any object's row (the oracle sees the unpadded points only)."""
    run_points(amd, dev, 5, n, precision)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("blocks", [(1, 0), (0, 2)], ids=lambda b: f"sb{b[0]}tb{b[1]}")
def test_points_other_latent_layouts(amd, dev, blocks, precision):
    """One latent slot and a texture-only layout: ``cols`` = 256 / 512 in the reduction (96 points: round-2 fp32)."""
    run_points(amd, dev, 3, 96, precision, blocks)


# ------------------------------------------------------------------ b. fused render backward (snr_render_bwd, mode 1)
def oracle_render(params, ro, rd, t, mode, S, n, zs, half, masks, wts, dt, lat=None, codes=None, lat_on=None):
    """Gradients of the fused render (white background; depths metric except per object) on the oracle in dtype ``dt``, latent terms as
    ``oracle_latent`` makes them: dict of d_rays_o, d_rays_d, d_t (per ray only), d_latent, d_shapecode, d_texturecode."""
    p = {k: v.to(dt) for k, v in params.items()}
    ro, rd = ro.to(dt).clone().requires_grad_(), rd.to(dt).clone().requires_grad_()
    t = t.to(dt).clone().requires_grad_() if mode == "per_ray" else t.to(dt)
    lat, sc, tc = oracle_latent(p, dt, lat, codes, lat_on)
    out = O.fused_render(p, ro, rd, t, mode, S, n, zs.to(dt), half.to(dt) if mode == "box" else None, latent=lat, relu_masks=masks,
                         white_bkgd=True, metric_z=mode != "per_object")
    sum((a * w.to(dt)).sum() for a, w in zip(out, wts)).backward()
    return dict(d_rays_o=ro.grad, d_rays_d=rd.grad, d_t=t.grad if mode == "per_ray" else None, d_latent=lat.grad, d_shapecode=grad_of(sc),
                d_texturecode=grad_of(tc))


# (z mode, S, rays per object, objects): rays x S per object, and the fp32 kernel (bf16x3: the split kernel, 32-point tiles, throughout)
RENDER_CASES = [
    ("per_object", 32, 1, 64),      # 32:   round-2 (32 % 64), 64 objects of one tile
    ("per_ray", 4, 8, 64),          # 32:   round-2; S = 4, 8 rays per object
    ("box", 4, 8, 5),               # 32:   round-2
    ("per_ray", 32, 3, 5),          # 96:   round-2, objects straddle 128-point workgroups
    ("box", 16, 6, 64),             # 96:   round-2
    ("per_object", 128, 1, 5),      # 128:  round-2 (S = 128 refused by the two-wave kernel)
    ("per_ray", 64, 2, 1),          # 128:  two-wave
    ("box", 128, 1, 64),            # 128:  round-2 (S = 128)
    ("per_object", 32, 33, 5),      # 1056 = 32*33: round-2, 33 tiles -> two levels
    ("per_ray", 8, 132, 1),         # 1056: round-2
    ("box", 64, 33, 5),             # 2112 = 64*33: two-wave, 33 tiles of 64 -> two levels (bf16x3: 66 tiles)
    ("per_object", 64, 33, 1),      # 2112: two-wave
    ("per_ray", 128, 33, 1),        # 4224 = 32*132: round-2 at S = 128
]


def render_inputs(mode, S, n, B, seed):
    N = B * n
    o, d, z = PD.box_rays(N, S, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    zs = torch.ones(B)
    half = torch.tensor([h + PD.H for h in PD.HALF]).expand(B, 3).contiguous()
    if mode == "per_object":
        t = torch.linspace(0.75, 2.25, S + 1)[:-1][None] + torch.rand(B, S, generator=g) * (1.5 / S)
    elif mode == "per_ray":
        t = z
    else:
        t = torch.rand(N, S, generator=g)
    s = obj_scale(B, n, seed + 2)
    wts = [torch.randn(N, 3, generator=g) * s[:, None], torch.randn(N, generator=g) * s, torch.randn(N, generator=g) * s]
    return o, d, t, zs, half, wts


@pytest.mark.parametrize("precision", PRECISIONS[:2] + ["auto"], ids=PREC_ID)
@pytest.mark.parametrize("case", RENDER_CASES, ids=lambda c: f"{c[0]}-S{c[1]}-n{c[2]}-B{c[3]}")
def test_render_latent_gradient_per_object(amd, dev, oracle_params, case, precision):
    ops = amd.ops
    mode, S, n, B = case
    o, d, t, zs, half, wts = render_inputs(mode, S, n, B, seed=S + 3 * n + 11 * B)
    sc, tc = codes(B, 50 + B + n)
    zmode = {"per_object": ops.Z_PER_OBJECT, "per_ray": ops.Z_PER_RAY, "box": ops.Z_BOX}[mode]
    cfg = ops.RenderCfg(S, zmode, n, 3, 1, white_bkgd=True, metric_z=mode != "per_object", box_half=half.to(dev) if mode == "box" else None)
    m = make_model(amd, dev, oracle_params, precision)
    lats = capture_latent(m)
    leaves = [x.to(dev).requires_grad_() for x in (o, d, t, sc, tc)]
    if mode != "per_ray":
        leaves[2] = t.to(dev)
    out = m.fused_render(leaves[0], leaves[1], leaves[2], torch.ones(B, device=dev), zs.to(dev), leaves[3], leaves[4], cfg)
    if precision == "auto":
        assert m.last_precision["forward"] == "bf16x3" and m.last_precision["backward"] == "bf16x3", m.last_precision
    masks = relu_bits_of(out[0], 3, 1, n_samples=S)
    sum((a * w.to(dev)).sum() for a, w in zip(out, wts)).backward()
    on = (lats[0].detach() > 0).cpu()
    r32, r64 = [oracle_render(oracle_params, o, d, t, mode, S, n, zs, half, masks, wts, dt, codes=(sc, tc), lat_on=on)
                for dt in (torch.float32, torch.float64)]
    bad = []
    for name, got in (("d_rays_o", leaves[0].grad), ("d_rays_d", leaves[1].grad), ("d_t", leaves[2].grad if mode == "per_ray" else None)):
        if got is not None:
            bad += check_per_ray(name, got, r32[name], r64[name])
    assert not bad, bad
    got = dict(d_latent=lats[0].grad, d_shapecode=leaves[3].grad, d_texturecode=leaves[4].grad)
    check_per_object([(k, v, r32[k], r64[k]) for k, v in got.items()], band_of(precision))


# ------------------------------------------------------------------ c. family B, split backward, small S
def family_b_scene(index, im_sz, S, seed):
    ob = O.synthetic_object(index)
    g = torch.Generator().manual_seed(seed)
    sc, tc = torch.randn(1, 256, generator=g) * 0.3, torch.randn(1, 256, generator=g) * 0.3
    jit = torch.rand(im_sz * im_sz, S, generator=g)
    return ob, sc, tc, jit


@pytest.mark.parametrize("precision", ["bf16x3", ("fp32", "bf16x3")], ids=PREC_ID)
@pytest.mark.parametrize("S,im_sz", [(64, 16), (128, 12), (32, 16), (16, 16), (8, 16), (4, 16), (64, 5), (16, 7)])
def test_box_render_and_gradients_small_split_mask_matched(amd, dev, oracle_params, S, im_sz, precision):
    """The split-backward twin of test_family_b_fused.py::test_box_render_and_gradients_small (same (S, im_sz) grid, padded 5x5 / 7x7 ray
    grids): every ray's gradient wrt its origin and direction (INCLUDING the path through its box bounds) by the per-ray rule, the pose's
    gradient through them, and the codes' -- on the function the forward's ReLU bits define."""
    ob, sc0, tc0, jit = family_b_scene(11, im_sz, S, 5)
    ro, vd = O.pixel_rays(ob["K"], ob["cam_pose"], ob["roi"], uv_steps=[im_sz, im_sz])
    N = ro.shape[0]
    g = torch.Generator().manual_seed(S + im_sz)
    w_rgb, w_d, w_a = torch.rand(N, 3, generator=g), torch.rand(N, generator=g) * 0.1, torch.rand(N, generator=g)
    model = make_model(amd, dev, oracle_params, precision)
    ro_d, vd_d = ro.to(dev).requires_grad_(), vd.to(dev).requires_grad_()
    sc, tc = sc0.to(dev).requires_grad_(), tc0.to(dev).requires_grad_()
    rend = amd.NeRFRenderer(n_samples=S, white_bkgd=True)
    out = rend._render(model, dev, ro_d, vd_d, ob["wlh"], sc, tc, False, True, jitter=jit)
    masks = relu_bits_of(out[0], 3, 1, n_samples=S)
    ((out[0] * w_rgb.to(dev)).sum() + (out[1] * w_d.to(dev)).sum() + (out[2] * w_a.to(dev)).sum()).backward()

    def oracle(dt):
        c = lambda x: x.to(dt)
        pose = c(ob["cam_pose"]).clone().requires_grad_()
        s, t = c(sc0).clone().requires_grad_(), c(tc0).clone().requires_grad_()
        o, v = O.pixel_rays(c(ob["K"]), pose, ob["roi"], uv_steps=[im_sz, im_sz])
        o.retain_grad()
        v.retain_grad()
        xyz, vv, z, hit = O.aabb_sampled_rays(o, v, ob["wlh"], S, c(jit))
        sig, rgb = O.decoder_forward({k: c(x) for k, x in oracle_params.items()}, xyz, vv, s, t, relu_masks=masks)
        r = O.composite(sig, rgb, z, white_bkgd=True)
        ((r[0] * c(w_rgb)).sum() + (r[1] * c(w_d)).sum() + (r[2] * c(w_a)).sum()).backward()
        return dict(d_rays_o=o.grad, d_rays_d=v.grad, d_pose=pose.grad, d_shapecode=s.grad, d_texturecode=t.grad, hit=hit)
    r32, r64 = oracle(torch.float32), oracle(torch.float64)
    assert bool(r64["hit"].any()) and bool((~r64["hit"]).any())
    bad = check_per_ray(f"d_rays_o S={S} {im_sz}x{im_sz}", ro_d.grad, r32["d_rays_o"], r64["d_rays_o"])
    bad += check_per_ray(f"d_rays_d S={S} {im_sz}x{im_sz}", vd_d.grad, r32["d_rays_d"], r64["d_rays_d"])
    assert not bad, bad
    # the pose's gradient: the kernel's per-ray gradients chained through the rays in float64
    pose = ob["cam_pose"].double().clone().requires_grad_()
    o, v = O.pixel_rays(ob["K"].double(), pose, ob["roi"], uv_steps=[im_sz, im_sz])
    ((o * ro_d.grad.cpu().double()).sum() + (v * vd_d.grad.cpu().double()).sum()).backward()
    check_per_object([("d_pose", pose.grad[None], r32["d_pose"][None], r64["d_pose"][None]),
                      ("d_shapecode", sc.grad, r32["d_shapecode"], r64["d_shapecode"]),
                      ("d_texturecode", tc.grad, r32["d_texturecode"], r64["d_texturecode"])], "bf16x3")


# ------------------------------------------------------------------ d. the workspace and the output at the C ABI
GUARD, SENTINEL = 1 << 16, 0xA5


def guarded_workspace(nbytes, dev):
    """Exactly ``nbytes`` of NaN followed by a 64 KiB guard of SENTINEL bytes."""
    assert nbytes % 4 == 0, nbytes
    ws = torch.full((nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    ws[:nbytes].view(torch.float32).fill_(float("nan"))
    return ws


def abi_bwd(amd, dev, mode, args, precision):
    """snr_decoder_bwd (mode 0: args = xyz, vd, lat, packed, masks, sig, d_sig, d_rgb, sb, tb) or snr_render_bwd (mode 1: args = the
    render operands, cfg, sig, rgbs, masks, d_rgb, d_depth, d_acc) through the C ABI with this helper's own buffers; returns d_latent,
    after asserting that the guard behind the requested workspace is intact."""
    ops, lib = amd.ops, amd._lib.lib()
    if mode == 0:
        xyz, vd, lat, packed, masks, sig, d_sig, d_rgb, sb, tb = args
        P, B = xyz.shape[0], lat.shape[0]
        nbytes = lib.snr_decoder_bwd_ws_bytes(P, P // B, sb, tb)
        ws = guarded_workspace(nbytes, dev)
        d_lat = torch.full_like(lat, float("nan"))
        d_xyz, d_dir = torch.empty_like(xyz), torch.empty_like(vd)
        code = ops.resolve_precision(precision, sb, tb, P // B, backward=True)
        with torch.cuda.device(dev):
            amd._lib.check(lib.snr_decoder_bwd(ops._p(xyz), ops._p(vd), ops._p(lat), ops._p(packed), ops._p(masks), ops._p(sig), ops._p(d_sig),
                                               ops._p(d_rgb), P, P // B, sb, tb, ops._p(d_lat), ops._p(d_xyz), ops._p(d_dir), None,
                                               ops._p(ws), nbytes, code, ops._stream(dev)), "snr_decoder_bwd")
    else:
        (ro, rd, t, xyz_div, zs, lat, packed, cfg), (sig, rgbs, masks, d_rgb, d_depth, d_acc) = args
        code = ops.resolve_precision(precision, cfg.shape_blocks, cfg.texture_blocks, cfg.rays_per_obj * cfg.n_samples, backward=True)
        a = ops._render_args(ro, rd, t, xyz_div, zs, lat, packed, cfg.frame, cfg.xyz_mul, cfg.z_mode, cfg.flags, cfg.rays_per_obj,
                             cfg.n_samples, cfg.shape_blocks, cfg.texture_blocks, code, box_half=cfg.box_half, rng=cfg.rng)
        nbytes = lib.snr_render_bwd_ws_bytes(C.byref(a))
        ws = guarded_workspace(nbytes, dev)
        d_lat = torch.full_like(lat, float("nan"))
        d_o, d_d = torch.empty_like(ro), torch.empty_like(rd)
        with torch.cuda.device(dev):
            amd._lib.check(lib.snr_render_bwd(C.byref(a), ops._p(sig), ops._p(rgbs), ops._p(masks), ops._p(d_rgb), ops._p(d_depth), ops._p(d_acc),
                                              ops._p(d_lat), ops._p(d_o), ops._p(d_d), None, ops._p(ws), nbytes, ops._stream(dev)), "snr_render_bwd")
    torch.cuda.synchronize(dev)
    guard = ws[nbytes:]
    assert bool((guard == SENTINEL).all()), f"{int((guard != SENTINEL).sum())} guard bytes behind the {nbytes}-byte workspace were written"
    assert bool(torch.isfinite(d_lat).all()), f"{int((~torch.isfinite(d_lat)).flatten(1).any(1).sum())} objects' rows not finite"
    return d_lat


def latent_input(B, nlat, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.relu(torch.randn(B, nlat, 256, generator=g) * 0.3)


@pytest.mark.parametrize("n,B,precision", [
    (32 * 1025, 1, "bf16x3"),        # three-level tree, 32-point tiles
    (32 * 1025, 1, "fp32"),          # three-level tree, round-2 fp32 (32*1025 % 64 != 0)
    (64 * 33, 3, "fp32"),            # two-wave fp32: 64-point tiles, the tree scratch starts at half the 32-point partials' size
    (32, 64, "bf16x3"), (32, 64, "fp32")], ids=lambda v: PREC_ID(v) if isinstance(v, (str, tuple)) else str(v))
def test_abi_decoder_workspace_and_output(amd, dev, oracle_params, n, B, precision):
    ops = amd.ops
    P = B * n
    g = torch.Generator().manual_seed(n + B)
    xyz, vd = torch.rand(P, 3, generator=g) * 2 - 1, F.normalize(torch.randn(P, 3, generator=g), dim=-1)
    lat = latent_input(B, 4, n * B)
    s = obj_scale(B, n, 7 * n + B)
    ws, wr = torch.randn(P, generator=g) * s, torch.randn(P, 3, generator=g) * s[:, None]
    m = make_model(amd, dev, oracle_params, precision)
    packed = m.packed_weights()
    xd, vdd, ld = xyz.to(dev), vd.to(dev), lat.to(dev)
    sig, _, masks = ops.decoder_fwd(xd, vdd, ld, packed, 3, 1, save_masks=True, precision=precision)
    d_lat = abi_bwd(amd, dev, 0, (xd, vdd, ld, packed, masks, sig, ws.to(dev), wr.to(dev), 3, 1), precision)
    mk = decode_relu_bits(masks, P, 3, 1)
    r32, r64 = [oracle_points(oracle_params, xyz, vd, mk, ws, wr, dt, lat=lat)[0] for dt in (torch.float32, torch.float64)]
    check_per_object([("d_latent", d_lat, r32, r64)], band_of(precision))


@pytest.mark.parametrize("case,precision", [
    (("per_ray", 4, 8, 64), "bf16x3"), (("per_ray", 4, 8, 64), "fp32"),     # 32 points per object, 64 objects
    (("box", 64, 33, 3), "fp32")],                                          # two-wave fp32 in render mode: 64-point tiles
    ids=lambda v: PREC_ID(v) if isinstance(v, str) else f"{v[0]}-S{v[1]}-n{v[2]}-B{v[3]}")
def test_abi_render_workspace_and_output(amd, dev, oracle_params, case, precision):
    ops = amd.ops
    mode, S, n, B = case
    o, d, t, zs, half, wts = render_inputs(mode, S, n, B, seed=5 * S + n)
    lat = latent_input(B, 4, S * B)
    zmode = {"per_ray": ops.Z_PER_RAY, "box": ops.Z_BOX}[mode]
    cfg = ops.RenderCfg(S, zmode, n, 3, 1, white_bkgd=True, metric_z=True, precision=precision, box_half=half.to(dev) if mode == "box" else None)
    m = make_model(amd, dev, oracle_params, precision)
    operands = (o.to(dev), d.to(dev), t.to(dev), torch.ones(B, device=dev), zs.to(dev), lat.to(dev), m.packed_weights(), cfg)
    fw = ops.render_fwd(*operands, save_for_bwd=True)
    d_lat = abi_bwd(amd, dev, 1, (operands, (fw[3], fw[4], fw[5], *[w.to(dev) for w in wts])), precision)
    mk = decode_relu_bits(fw[5], B * n * S, 3, 1)
    r32, r64 = [oracle_render(oracle_params, o, d, t, mode, S, n, zs, half, mk, wts, dt, lat=lat)["d_latent"]
                for dt in (torch.float32, torch.float64)]
    check_per_object([("d_latent", d_lat, r32, r64)], band_of(precision))


# ------------------------------------------------------------------ e. many objects
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_more_objects_than_a_grid_row_holds(amd, dev, oracle_params, precision):
    """70 000 objects of 32 points (2.24 M points, 4 latent slots, 287 MB of partials): n_obj above 65 535, the reduction's grid.y.  Two
    outcomes are correct: every object's row right, or SnrError.  Sampled objects against the float64 oracle; every row against the same
    objects launched in two batches of fewer than 65 536 objects (the reduction is deterministic: the rows must be bit for bit the same)."""
    ops = amd.ops
    from supnerf_amd._lib import SnrError
    B, n = 70000, 32
    P = B * n
    gd = torch.Generator(device=dev).manual_seed(3)
    xyz = torch.rand(P, 3, device=dev, generator=gd) * 2 - 1
    vd = F.normalize(torch.randn(P, 3, device=dev, generator=gd), dim=-1)
    lat = torch.relu(torch.randn(B, 4, 256, device=dev, generator=gd) * 0.3)
    s = (10.0 ** (torch.rand(B, device=dev, generator=gd) * 3 - 1.5)).repeat_interleave(n)
    ws, wr = torch.randn(P, device=dev, generator=gd) * s, torch.randn(P, 3, device=dev, generator=gd) * s[:, None]
    m = make_model(amd, dev, oracle_params, precision)
    packed = m.packed_weights()
    lat_l = lat.clone().requires_grad_()
    sig, rgb = ops.DecoderPoints.apply(xyz, vd, lat_l, packed, 3, 1, precision)
    masks = sig.grad_fn.saved_tensors[4]                             # (ops.DecoderPoints saves xyz, viewdir, latent, packed, masks, sig)
    try:
        ((sig * ws).sum() + (rgb * wr).sum()).backward()
    except SnrError as e:
        print(f"[{B} objects] SnrError: {e}")
        return
    d_lat = lat_l.grad
    print(f"[{B} objects, {precision}] the backward returned")
    assert bool(torch.isfinite(d_lat).all()), int((~torch.isfinite(d_lat)).flatten(1).any(1).sum())
    sig_s = sig.detach()
    per_tile = masks.numel() // B                                    # one tile per object
    # every row: the same objects in two launches whose reductions have fewer than 65 536 grid rows
    for o0, o1 in ((0, 32768), (32768, B)):
        sl = slice(o0 * n, o1 * n)
        part = ops.decoder_bwd(xyz[sl], vd[sl], lat[o0:o1], packed, masks[o0 * per_tile:o1 * per_tile], sig_s[sl], ws[sl], wr[sl], 3, 1,
                               need_xyz=False, need_dir=False, precision=ops.resolve_precision(precision, 3, 1, n, backward=True))[0]
        diff = (part != d_lat[o0:o1]).flatten(1).any(1)
        assert not bool(diff.any()), f"{int(diff.sum())} objects differ from the batched launch, first {(torch.nonzero(diff).flatten()[:8] + o0).tolist()}"
    # sampled objects against float64
    objs = [0, 1, 65534, 65535, 65536, B - 1]
    idx = torch.cat([torch.arange(b * n, (b + 1) * n) for b in objs]).to(dev)
    mk = torch.cat([masks[b * per_tile:(b + 1) * per_tile] for b in objs])
    mk = decode_relu_bits(mk, len(objs) * n, 3, 1)
    args = [x[idx].cpu() for x in (xyz, vd)] + [mk] + [x[idx].cpu() for x in (ws, wr)]
    r32, r64 = [oracle_points(oracle_params, *args, dt, lat=lat[objs].cpu())[0] for dt in (torch.float32, torch.float64)]
    check_per_object([("d_latent", d_lat[objs], r32, r64)], band_of(precision), objects=objs)
