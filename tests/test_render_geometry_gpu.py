"""The fused render's ray geometry -- per-object xyz_div / z_scale / box_half, xyz_mul = 0.9, frames that are not the identity -- on every
render kernel, against the float32 / float64 oracle on the ReLU bits the kernel saved.  The launches are those of
tests/render_geometry_cases.py; tests/test_render_geometry_cpu.py shows that the bands applied here see a constant taken from the
neighbouring object, a transposed frame and a dropped xyz_mul on each of them.

Raw operators (``ops.render_fwd`` + ``ops.render_bwd(need_latent=False)``, fp32): nothing pads the ragged objects, so the exact-fp32
kernels meet object boundaries inside a workgroup -- ``decoder_fwd16_kernel`` (WAVES = 4: 64 points per workgroup; S = 128: WAVES = 8, one
ray per workgroup) and, without latent partials, ``decoder_bwd16_kernel<1>`` for S <= 64 (csrc/snr_mlp16_bwd.hip
``snr_fp32_bwd16_supported_``), the 32x32 ``decoder_bwd_kernel`` for S = 128.  Both two-waves kernels take the object of a lane from
``point_id`` (csrc/snr_mlp16_core.hpp).
Module route (``model.fused_render``, codes, rays and per-ray depths as leaves; fp32, and bf16x3 / auto where the padded objects are whole
32-point tiles): padding (``ops.pad_render_inputs``), the latent gradient and its reduction under the same geometry.  The two cases with
one ray per object are the ones a (B,) z_scale padded like a per-ray table broke: objects 1 and 2 came back with depth 0 and acc_trans 1
(per-ray depths) or NaN throughout (box sampling).

Room when written (MI355X): no tensor above 0.18 of its band, no ray above 0.20 of the per-ray rule, ``ops.encode`` at most 0.77 of its bound."""
import pytest
import torch

import render_geometry_cases as RG
from oracle import supnerf_oracle as O
from oracle_bands import amd, band_of, capture_latent, check_all, check_per_object, check_per_ray, dev, make_model  # noqa: F401  (amd, dev: fixtures)
from relu_bits import decode_relu_bits, relu_bits_of

pytestmark = pytest.mark.gpu

RAW_RUNS = [r for r in RG.RUNS if r[0] == "raw"]
MODULE_RUNS = [r for r in RG.RUNS if r[0] == "module"]
EPS = 2.0 ** -23


def cfg_of(ops, c, dev, precision, blocks=(3, 1)):
    zmode = {"shared": ops.Z_SHARED, "per_object": ops.Z_PER_OBJECT, "per_ray": ops.Z_PER_RAY, "box": ops.Z_BOX}[c.mode]
    return ops.RenderCfg(c.S, zmode, c.n, blocks[0], blocks[1], frame=tuple(c.frame.flatten().tolist()), xyz_mul=c.xyz_mul, white_bkgd=True,
                         metric_z=True, precision=precision, box_half=c.box_half.to(dev) if c.mode == "box" else None)


def hold(tag, got, r32, r64, band, per_object=()):
    """Outputs in their band, every ray's gradient by the per-ray rule, every object's rows in the band."""
    check_all([(f"{tag} {k}", got[k], r32[k], r64[k]) for k in ("rgb", "depth", "acc")], band[0])
    bad = []
    for k in ("d_rays_o", "d_rays_d", "d_t"):
        assert (got[k] is None) == (r64[k] is None), k
        if got[k] is not None:
            bad += check_per_ray(f"{tag} {k}", got[k], r32[k], r64[k])
    assert not bad, bad
    if per_object:
        check_per_object([(f"{tag} {k}", got[k], r32[k], r64[k]) for k in per_object], band[1])


# ------------------------------------------------------------------ a. the raw operators: ragged objects, unpadded
@pytest.mark.parametrize("run", RAW_RUNS, ids=RG.RUN_ID)
def test_raw_operators_hold_the_geometry(amd, dev, oracle_params, run):
    ops = amd.ops
    _, case, fname = run
    c = RG.build(case, fname)
    N = c.B * c.n
    m = make_model(amd, dev, oracle_params, "fp32")
    cfg = cfg_of(ops, c, dev, "fp32")
    operands = (c.rays_o.to(dev), c.rays_d.to(dev), c.t_vals.to(dev), c.xyz_div.to(dev), c.z_scale.to(dev), c.latent.to(dev), m.packed_weights(), cfg)
    fw = ops.render_fwd(*operands, save_for_bwd=True)
    up = [w.to(dev) for w in c.wts]
    need_t = c.mode == "per_ray"
    bw = ops.render_bwd(*operands, fw[3], fw[4], fw[5], *up, need_t=need_t, need_latent=False)
    again = ops.render_bwd(*operands, fw[3], fw[4], fw[5], *up, need_t=need_t, need_latent=False)
    assert bw[3] is None
    for name, a, b in zip(("d_rays_o", "d_rays_d", "d_t"), bw, again):
        assert (a is None and b is None) or torch.equal(a, b), f"{name}: two backward launches differ"
    masks = decode_relu_bits(fw[5], N * c.S, 3, 1)
    r32, r64 = [RG.oracle(oracle_params, c, dt, masks=masks, latent=c.latent) for dt in (torch.float32, torch.float64)]
    got = dict(rgb=fw[0], depth=fw[1], acc=fw[2], d_rays_o=bw[0], d_rays_d=bw[1], d_t=bw[2])
    hold(RG.RUN_ID(run), got, r32, r64, ("fp32", "fp32"))


# ------------------------------------------------------------------ b. the module route: padding, latent gradient, reduction
@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "auto"])
@pytest.mark.parametrize("run", MODULE_RUNS, ids=RG.RUN_ID)
def test_module_route_holds_the_geometry(amd, dev, oracle_params, run, precision):
    ops = amd.ops
    _, case, fname = run
    c = RG.build(case, fname)
    per_obj = (ops._tile_pad(c.n, c.S) or c.n) * c.S
    # every case of the list pads to whole 32-point tiles, so the split kernels must take it: nothing is skipped here
    assert ops.split_supported(3, 1, per_obj), (case, per_obj)
    m = make_model(amd, dev, oracle_params, precision)
    lats = capture_latent(m)
    ro, rd, t, sc, tc = [x.to(dev).requires_grad_() for x in (c.rays_o, c.rays_d, c.t_vals, *c.codes)]
    if c.mode != "per_ray":
        t = c.t_vals.to(dev)
    out = m.fused_render(ro, rd, t, c.xyz_div.to(dev), c.z_scale.to(dev), sc, tc, cfg_of(ops, c, dev, None))
    ran = (m.last_precision["forward"], m.last_precision["backward"])
    want = "fp32" if precision == "fp32" else "bf16x3"
    assert ran == (want, want), (precision, m.last_precision)
    masks = relu_bits_of(out[0], 3, 1, n_samples=c.S)
    sum((a * w.to(dev)).sum() for a, w in zip(out, c.wts)).backward()
    on = (lats[0].detach() > 0).cpu()
    r32, r64 = [RG.oracle(oracle_params, c, dt, masks=masks, lat_on=on) for dt in (torch.float32, torch.float64)]
    got = dict(rgb=out[0], depth=out[1], acc=out[2], d_rays_o=ro.grad, d_rays_d=rd.grad, d_t=t.grad if c.mode == "per_ray" else None,
               d_latent=lats[0].grad, d_shapecode=sc.grad, d_texturecode=tc.grad)
    hold(f"{RG.RUN_ID(run)} {precision}", got, r32, r64, (ran[0], band_of(ran[1])), per_object=("d_latent", "d_shapecode", "d_texturecode"))


# ------------------------------------------------------------------ c. the sample points alone
def geometry_fp32(c):
    """The part of ``make_sample`` in front of the geometry, in the kernel's own fp32 steps on the CPU (IEEE: the same bits): the
    sampling-frame origin o (N,3), depth t (N,S) and point p = o + t d (N,S,3), and the hit mask ("box").  For "box" that is the slab
    test and the stratified depths (tests/test_special_rays_gpu.py holds those to the kernel bit for bit)."""
    N = c.B * c.n
    obj = torch.arange(N) // c.n
    o, d, hit = c.rays_o, c.rays_d, None
    if c.mode == "box":
        o = o / c.z_scale[obj][:, None]
        h = c.box_half[obj]
        near, far, hit = O.slab_intersect(o, d, -h, h)
        minus1 = torch.full_like(near, -1.0)
        t = O.unit_interval_samples(torch.where(hit, near, minus1)[:, None], torch.where(hit, far, minus1)[:, None], c.S, c.t_vals)
    else:
        t = {"shared": lambda: c.t_vals[None].expand(N, c.S), "per_object": lambda: c.t_vals[obj], "per_ray": lambda: c.t_vals}[c.mode]()
    return o, t, o[:, None, :] + t[:, :, None] * d[:, None, :], hit


@pytest.mark.parametrize("run", RAW_RUNS, ids=RG.RUN_ID)
def test_encode_places_every_sample(amd, dev, run):
    """``ops.encode`` (``encode_kernel``: the same ``make_sample``) component by component against the float64 geometry
    M ((p / xyz_div[b]) xyz_mul), M d and |t d| z_scale[b]: within 4 x 2^-23 x sum_i |M_ki| |q_i|, q = (p / xyz_div[b]) xyz_mul -- seven
    fp32 roundings (divide, scale, three products, two sums), each at most 2^-24 of the running magnitude, which sum_i |M_ki| |q_i| bounds.
    p, the fp32 point in front of the divide, is ``geometry_fp32``'s; with per-ray / per-object / shared depths (t is an input) the
    float64 point o + t d is held as well, with the two roundings of its own added: 2^-24 (|t d_i| + |p_i|) in front of the scale."""
    ops = amd.ops
    _, case, fname = run
    c = RG.build(case, fname)
    N = c.B * c.n
    obj = torch.arange(N) // c.n
    box = c.mode == "box"
    cfg = cfg_of(ops, c, dev, None, blocks=(0, 0))
    out = ops.encode(c.rays_o.to(dev), c.rays_d.to(dev), c.t_vals.to(dev), c.xyz_div.to(dev), c.z_scale.to(dev), cfg, want_hit=box)
    xyz, vd, z = [x.cpu().double() for x in out[:3]]
    o32, t32, p32, hit = geometry_fp32(c)
    M, d = c.frame.double(), c.rays_d.double()
    scale = (torch.ones(N, dtype=torch.float64) if box else 1.0 / c.xyz_div.double()[obj]) * c.xyz_mul
    if box:
        assert torch.equal(out[3].cpu(), hit), torch.nonzero(out[3].cpu() != hit).flatten().tolist()

    def frame_bound(q):
        return 4 * EPS * (q.abs() @ M.abs().T)

    def worst(name, got, want, bound):
        r = ((got - want).abs() / bound)
        print(f"[encode {RG.RUN_ID(run)}] {name}: worst error / bound {float(r.max()):.3f}")
        assert bool(torch.isfinite(got).all()) and float(r.max()) <= 1.0, (name, float(r.max()), torch.nonzero(r > 1)[:8].tolist())

    q = p32.double() * scale[:, None, None]
    worst("xyz", xyz, q @ M.T, frame_bound(q))
    worst("viewdir", vd, (d @ M.T)[:, None, :].expand(N, c.S, 3), frame_bound(d)[:, None, :].expand(N, c.S, 3))
    zc = (t32.double()[:, :, None] * d[:, None, :]).norm(dim=-1) * c.z_scale.double()[obj][:, None]
    worst("metric depth", z, zc, 4 * EPS * zc)
    if not box:
        td = t32.double()[:, :, None] * d[:, None, :]
        p64 = o32.double()[:, None, :] + td
        q64 = p64 * scale[:, None, None]
        extra = 0.5 * EPS * ((td.abs() + p64.abs()) * scale[:, None, None]) @ M.abs().T
        worst("xyz from o + t d in float64", xyz, q64 @ M.T, frame_bound(q64) + extra * (1 + 8 * EPS))
