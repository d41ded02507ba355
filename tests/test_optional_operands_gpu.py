"""The optional operands of the five backward entry points on the kernels: NULL upstream gradients, dropped outputs, and every upstream
path alone against float64.  The launches, subsets and the three contracts are those of tests/optional_operand_cases.py;
tests/test_optional_operands_cpu.py measures on the oracle how much of the usual combined loss each path is and shows that the single-path
checks applied here notice a path that is 0.8 % wrong.

a. ``snr_render_bwd``, raw (``ops.render_fwd(save_for_bwd=True)`` + ``ops.render_bwd``) and through ``model.fused_render`` (a loss that
   reads one or two outputs: ``FusedRender`` does not materialise the others' gradients, so the kernel gets NULL), fp32 and bf16x3.
b. ``snr_decoder_bwd``: d_sigmas / d_rgbs NULL, every output subset, on the 16x16, the 32x32 (``layer_grads``) and the split kernel;
   the sigma-only launch with d_rgbs NULL is ``ops.density_bwd`` bit for bit.
c. ``snr_density_bwd``, d. ``snr_composite_bwd``, e. ``snr_scene_composite_bwd``: the same contracts where they apply.

Comparisons that are NOT bit for bit, and why: exact fp32 with 96 (render: shared-S8-n12-B2) or 96 / 32 (decoder without ``layer_grads``)
points per object runs ``decoder_bwd16_kernel`` without d_latent and the 32x32 ``decoder_bwd_kernel`` with it
(``snr_fp32_bwd16_supported_``); the two sum in another order (tests/test_hip_kernels.py::test_fp32_backward_kernels_agree holds them to
2e-6).  There the launch without d_latent is held to the fp32 band against float64 instead, and outputs are always compared with the full
launch of the same ``need_latent``.  Everything else is ``torch.equal``.

Room when written (MI355X): every comparison expected to be the same bits is; no all-NULL launch leaves a non-zero or unwritten element.
Worst single-path error over its band (tensors and per-object rows) / worst ray over the per-ray rule, all on an acc-only loss of
shared-S8-n12-B2 unless named: render raw fp32 0.10 / 0.13, bf16x3 0.22 / 0.18; render module fp32 0.06 / 0.13, bf16x3 0.15 / 0.18;
decoder fp32 0.07 (192/2 sigma-only), bf16x3 0.23 (96/3 rgb-only); composite 0.05 (S64 shared white, depth-only).  The two exact-fp32
kernels differ by 6.6e-7 (d_rays_o) and 1.5e-7 (d_rays_d) of the largest entry on shared-S8-n12-B2, the 16x16 launch at 0.06 of the
per-ray rule; on the decoder it is at 0.04 of the fp32 band."""
import pytest
import torch

import optional_operand_cases as OC
import render_geometry_cases as RG
from oracle_bands import amd, band_of, check_all, check_per_ray, dev, in_band, make_model  # noqa: F401  (amd, dev: fixtures)
from relu_bits import decode_relu_bits, relu_bits_of

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "bf16x3"]
SB, TB = OC.SB, OC.TB
NEED_OF = dict(zip(OC.RENDER_OUTPUTS, ("need_o", "need_d", "need_t", "need_latent")))


def same_bits(tag, got, want, keys):
    for k in keys:
        assert OC.written(got[k]), f"{tag} {k}: elements the kernel did not write"
        assert torch.equal(got[k], want[k]), f"{tag} {k}: differs by {float((got[k] - want[k]).abs().max()):.3e}"


# ------------------------------------------------------------------ a. snr_render_bwd, raw
_RAW = {}


def raw_launch(amd, dev, params, case, precision):
    """The launch, its device operands, what the forward saved, the decoded ReLU bits and the three upstream weights; one forward per
    (launch, precision) for the whole module."""
    if (case, precision) not in _RAW:
        ops = amd.ops
        c = RG.build(case)
        m = make_model(amd, dev, params, precision)
        operands = (c.rays_o.to(dev), c.rays_d.to(dev), c.t_vals.to(dev), c.xyz_div.to(dev), c.z_scale.to(dev), c.latent.to(dev), m.packed_weights(),
                    OC.render_cfg(ops, c, dev, precision))
        fw = ops.render_fwd(*operands, save_for_bwd=True)
        _RAW[case, precision] = c, operands, fw[3:6], decode_relu_bits(fw[5], c.B * c.n * c.S, SB, TB), tuple(w.to(dev) for w in c.wts)
    return _RAW[case, precision]


def raw_bwd(ops, operands, saved, up, **need):
    with OC.nan_filled_outputs(ops):
        return dict(zip(OC.RENDER_OUTPUTS, ops.render_bwd(*operands, *saved, *up, **need)))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", OC.RENDER_LAUNCHES, ids=OC.LAUNCH_ID)
def test_render_null_upstream_is_a_zero_upstream(amd, dev, oracle_params, case, precision):
    ops = amd.ops
    c, operands, saved, _, up = raw_launch(amd, dev, oracle_params, case, precision)
    need = OC.render_output_subsets(c)["full"]
    keys = [k for k in OC.RENDER_OUTPUTS if need[NEED_OF[k]]]
    for s in OC.SUBSETS:
        null = raw_bwd(ops, operands, saved, OC.keep(up, s), **need)
        zero = raw_bwd(ops, operands, saved, OC.keep(up, s, torch.zeros_like), **need)
        same_bits(f"{OC.LAUNCH_ID(case)} {precision} upstream {OC.SUBSET_ID(s)}", null, zero, keys)
        assert all(float(null[k].abs().max()) > 0 for k in keys)
    nothing = raw_bwd(ops, operands, saved, (None, None, None), **need)
    for k in keys:
        assert OC.written(nothing[k]) and OC.zeros_equal(nothing[k]), f"{k}: no upstream gradient at all, yet not exactly zero"


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", OC.RENDER_LAUNCHES, ids=OC.LAUNCH_ID)
def test_render_dropping_an_output_changes_no_other(amd, dev, oracle_params, case, precision):
    ops = amd.ops
    c, operands, saved, masks, up = raw_launch(amd, dev, oracle_params, case, precision)
    tag = f"{OC.LAUNCH_ID(case)} {precision}"
    subs = OC.render_output_subsets(c)
    got = {name: raw_bwd(ops, operands, saved, up, **flags) for name, flags in subs.items()}
    base = {True: got["full"], False: got["no_need_latent"]}            # the same need_latent: the same kernel
    for name, flags in subs.items():
        keys = [k for k in OC.RENDER_OUTPUTS if flags[NEED_OF[k]]]
        assert all(got[name][k] is None for k in OC.RENDER_OUTPUTS if k not in keys), name
        same_bits(f"{tag} {name}", got[name], base[flags["need_latent"]], keys)
    rays = [k for k in OC.RENDER_OUTPUTS[:3] if got["full"][k] is not None]
    if precision == "fp32" and OC.fp32_latent_toggle_changes_kernel(c.S * c.n, c.S):
        # decoder_bwd16_kernel (no d_latent) against decoder_bwd_kernel (with it): another order of the sums, so both launches are held to
        # the per-ray rule against float64 on the combined loss instead of to the same bits
        r32, r64 = [RG.oracle(oracle_params, c, dt, masks=masks, latent=c.latent) for dt in (torch.float32, torch.float64)]
        bad = []
        for name in ("full", "no_need_latent"):
            for k in rays:
                bad += check_per_ray(f"{tag} {name} {k}", got[name][k], r32[k], r64[k])
        assert not bad, bad
        print(f"[optional operands] {tag}: 16x16 against 32x32 kernel, largest difference "
              + ", ".join(f"{k} {float((got['full'][k] - got['no_need_latent'][k]).abs().max() / got['full'][k].abs().max()):.1e}" for k in rays)
              + f"; worst ray {max(OC.ray_rule_ratio(got['no_need_latent'][k], r32[k], r64[k]) for k in rays):.3f} of the per-ray rule")
    else:
        same_bits(f"{tag} without d_latent", got["no_need_latent"], got["full"], rays)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("path", OC.SINGLES, ids=OC.SUBSET_ID)
@pytest.mark.parametrize("case", OC.RENDER_LAUNCHES, ids=OC.LAUNCH_ID)
def test_render_each_path_alone_against_float64(amd, dev, oracle_params, case, path, precision):
    ops = amd.ops
    c, operands, saved, masks, up = raw_launch(amd, dev, oracle_params, case, precision)
    got = raw_bwd(ops, operands, saved, OC.keep(up, path), **OC.render_output_subsets(c)["full"])
    r32, r64 = [RG.oracle(oracle_params, OC.single_path(c, path), dt, masks=masks, latent=c.latent) for dt in (torch.float32, torch.float64)]
    OC.hold_render_path(f"render raw {OC.LAUNCH_ID(case)} {precision} {OC.SUBSET_ID(path)}-only", got, r32, r64, band_of(precision),
                        reaches_texture=path == (0,))


# ------------------------------------------------------------------ a. snr_render_bwd behind model.fused_render
MODULE_OUTPUTS = OC.RENDER_OUTPUTS + ("d_shapecode", "d_texturecode")
LEAVES = ("o", "d", "t", "codes")


def model_keeping_latent(amd, dev, params, precision):
    """The module, and the list its ``latent_terms`` appends every result to -- with its gradient retained where it has one."""
    m, seen = make_model(amd, dev, params, precision), []
    plain = m.latent_terms

    def latent_terms(sc, tc):
        z = plain(sc, tc)
        if z.requires_grad:
            z.retain_grad()
        seen.append(z)
        return z
    m.latent_terms = latent_terms
    return m, seen


def module_run(amd, dev, model, c, precision, read, zero_weighted=(), leaves=LEAVES, want_masks=False):
    """``model.fused_render`` on the launch, then the backward of the loss that reads the outputs ``read`` (indices into PATHS) with the
    launch's weights, plus the outputs ``zero_weighted`` times a zeros tensor (autograd then delivers explicit zeros where it delivers
    None otherwise).  ``leaves``: which inputs require a gradient.  Returns the gradients over MODULE_OUTPUTS (None where there is none),
    the saved ReLU bits and the latent terms' z > 0."""
    m, seen = model
    leaf = lambda x, on: x.to(dev).requires_grad_(on)                                        # noqa: E731
    ro, rd, t = leaf(c.rays_o, "o" in leaves), leaf(c.rays_d, "d" in leaves), leaf(c.t_vals, "t" in leaves and c.mode == "per_ray")
    sc, tc = [leaf(x, "codes" in leaves) for x in c.codes]
    out = m.fused_render(ro, rd, t, c.xyz_div.to(dev), c.z_scale.to(dev), sc, tc, OC.render_cfg(amd.ops, c, dev, None))
    assert (m.last_precision["forward"], m.last_precision["backward"]) == (precision, precision), m.last_precision
    masks = relu_bits_of(out[0], SB, TB, n_samples=c.S) if want_masks else None
    loss = sum((out[i] * c.wts[i].to(dev)).sum() for i in read) + sum((out[i] * torch.zeros_like(out[i])).sum() for i in zero_weighted)
    loss.backward()
    lat = seen[-1]
    return dict(zip(MODULE_OUTPUTS, (ro.grad, rd.grad, t.grad, lat.grad if lat.requires_grad else None, sc.grad, tc.grad))), masks, (lat.detach() > 0).cpu()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", OC.RENDER_LAUNCHES, ids=OC.LAUNCH_ID)
def test_module_unread_outputs_are_zero_weighted_outputs(amd, dev, oracle_params, case, precision):
    """A loss that does not read an output (a NULL pointer at the kernel) against the same loss plus that output times zeros."""
    c = RG.build(case)
    model = model_keeping_latent(amd, dev, oracle_params, precision)
    for s in OC.SUBSETS:
        unread = tuple(i for i in range(3) if i not in s)
        null = module_run(amd, dev, model, c, precision, s)[0]
        zero = module_run(amd, dev, model, c, precision, s, zero_weighted=unread)[0]
        keys = [k for k in MODULE_OUTPUTS if zero[k] is not None]
        assert set(keys) == set(MODULE_OUTPUTS) - (set() if c.mode == "per_ray" else {"d_t"})
        assert all(null[k] is not None for k in keys)
        same_bits(f"module {OC.LAUNCH_ID(case)} {precision} reads {OC.SUBSET_ID(s)}", null, zero, keys)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", OC.RENDER_LAUNCHES, ids=OC.LAUNCH_ID)
def test_module_dropping_an_input_gradient_changes_no_other(amd, dev, oracle_params, case, precision):
    """``needs_input_grad`` becomes need_o / need_d / need_t / need_latent: every gradient against the launch that asks for everything else
    with the same ``need_latent`` (the same kernel).  The two kernels of exact fp32 are compared in the raw test above."""
    c = RG.build(case)
    model = model_keeping_latent(amd, dev, oracle_params, precision)
    live = [x for x in LEAVES if x != "t" or c.mode == "per_ray"]
    subsets = {"full": tuple(live), **{"no_" + x: tuple(y for y in live if y != x) for x in live}, **{"only_" + x: (x,) for x in live if x != "codes"}}
    got = {name: module_run(amd, dev, model, c, precision, (0, 1, 2), leaves=lv)[0] for name, lv in subsets.items()}
    base = {True: got["full"], False: got["no_codes"]}
    owner = dict(d_rays_o="o", d_rays_d="d", d_t="t", d_latent="codes", d_shapecode="codes", d_texturecode="codes")
    for name, lv in subsets.items():
        keys = [k for k in MODULE_OUTPUTS if owner[k] in lv]
        assert all(got[name][k] is None for k in MODULE_OUTPUTS if k not in keys), name
        same_bits(f"module {OC.LAUNCH_ID(case)} {precision} {name}", got[name], base["codes" in lv], keys)
    if not (precision == "fp32" and OC.fp32_latent_toggle_changes_kernel(c.S * c.n, c.S)):
        same_bits(f"module {OC.LAUNCH_ID(case)} {precision} without the codes", got["no_codes"], got["full"],
                  [k for k in OC.RENDER_OUTPUTS[:3] if got["full"][k] is not None])


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("path", OC.SINGLES, ids=OC.SUBSET_ID)
@pytest.mark.parametrize("case", OC.RENDER_LAUNCHES, ids=OC.LAUNCH_ID)
def test_module_each_path_alone_against_float64(amd, dev, oracle_params, case, path, precision):
    c = RG.build(case)
    got, masks, on = module_run(amd, dev, model_keeping_latent(amd, dev, oracle_params, precision), c, precision, path, want_masks=True)
    r32, r64 = [RG.oracle(oracle_params, OC.single_path(c, path), dt, masks=masks, lat_on=on) for dt in (torch.float32, torch.float64)]
    OC.hold_render_path(f"render module {OC.LAUNCH_ID(case)} {precision} {OC.SUBSET_ID(path)}-only", got, r32, r64, band_of(precision),
                        reaches_texture=path == (0,), per_object=("d_latent", "d_shapecode", "d_texturecode"))


# ------------------------------------------------------------------ b. snr_decoder_bwd
_DEC = {}


def decoder_launch(amd, dev, params, P, B, precision):
    if (P, B, precision) not in _DEC:
        ops = amd.ops
        cpu = OC.decoder_inputs(P, B)
        xyz, vd, lat = [x.to(dev) for x in cpu[:3]]
        packed = make_model(amd, dev, params, precision).packed_weights()
        sig, _, mk = ops.decoder_fwd(xyz, vd, lat, packed, SB, TB, save_masks=True, precision=precision)
        _DEC[P, B, precision] = cpu, (xyz, vd, lat, packed, mk, sig), decode_relu_bits(mk, P, SB, TB), tuple(w.to(dev) for w in cpu[3])
    return _DEC[P, B, precision]


def decoder_bwd(ops, args, up, kernel, **need):
    """(outputs over DECODER_OUTPUTS, the layer_grads dump or None).  The dump starts as zeros: rgb.0's slot has 128 columns nobody writes."""
    precision, layer_grads = kernel
    dump = torch.zeros(SB + TB + 4, args[0].shape[0], 256, device=args[0].device) if layer_grads else None
    with OC.nan_filled_outputs(ops):
        out = ops.decoder_bwd(*args, up[0], up[1], SB, TB, precision=precision, layer_grads=dump, **need)
    return dict(zip(OC.DECODER_OUTPUTS, out)), dump


@pytest.mark.parametrize("kernel", OC.DECODER_KERNELS, ids=OC.KERNEL_ID)
@pytest.mark.parametrize("P,B", OC.DECODER_SHAPES)
def test_decoder_null_upstream_is_a_zero_upstream(amd, dev, oracle_params, P, B, kernel):
    ops = amd.ops
    _, args, _, up = decoder_launch(amd, dev, oracle_params, P, B, kernel[0])
    for s in ((0,), (1,), (0, 1)):
        null, dump_n = decoder_bwd(ops, args, OC.keep(up, s), kernel)
        zero, dump_z = decoder_bwd(ops, args, OC.keep(up, s, torch.zeros_like), kernel)
        same_bits(f"decoder {P}/{B} {OC.KERNEL_ID(kernel)} upstream {s}", null, zero, OC.DECODER_OUTPUTS)
        assert float(null["d_xyz"].abs().max()) > 0
        if dump_n is not None:
            assert torch.equal(dump_n, dump_z) and float(dump_n.abs().max()) > 0
    nothing, dump = decoder_bwd(ops, args, (None, None), kernel)
    for k in OC.DECODER_OUTPUTS:
        assert OC.written(nothing[k]) and OC.zeros_equal(nothing[k]), k
    assert dump is None or OC.zeros_equal(dump)


@pytest.mark.parametrize("kernel", OC.DECODER_KERNELS, ids=OC.KERNEL_ID)
@pytest.mark.parametrize("P,B", OC.DECODER_SHAPES)
def test_decoder_dropping_an_output_changes_no_other(amd, dev, oracle_params, P, B, kernel):
    ops = amd.ops
    cpu, args, masks, up = decoder_launch(amd, dev, oracle_params, P, B, kernel[0])
    tag = f"decoder {P}/{B} {OC.KERNEL_ID(kernel)}"
    subs = OC.decoder_output_subsets()
    got = {name: decoder_bwd(ops, args, up, kernel, **flags)[0] for name, flags in subs.items()}
    base = {True: got["full"], False: got["no_need_latent"]}
    need_of = dict(d_latent="need_latent", d_xyz="need_xyz", d_dir="need_dir")
    for name, flags in subs.items():
        keys = [k for k in OC.DECODER_OUTPUTS if flags[need_of[k]]]
        assert all(got[name][k] is None for k in OC.DECODER_OUTPUTS if k not in keys), name
        same_bits(f"{tag} {name}", got[name], base[flags["need_latent"]], keys)
    if kernel[0] == "fp32" and OC.fp32_latent_toggle_changes_kernel(P // B, layer_grads=kernel[1]):
        # 16x16 without d_latent, 32x32 with it: the fp32 band against float64 instead of the same bits
        r32, r64 = [OC.oracle_decoder(oracle_params, *cpu[:3], masks, cpu[3], dt) for dt in (torch.float32, torch.float64)]
        for name in ("full", "no_need_latent"):
            check_all([(f"{tag} {name} {k}", got[name][k], r32[k], r64[k]) for k in ("d_xyz", "d_dir")], "fp32")
        print(f"[optional operands] {tag}: 16x16 against 32x32 kernel, worst "
              f"{max(in_band(got['no_need_latent'][k], r32[k], r64[k], 'fp32')[1] for k in ('d_xyz', 'd_dir')):.3f} of the band")
    else:
        same_bits(f"{tag} without d_latent", got["no_need_latent"], got["full"], ("d_xyz", "d_dir"))


@pytest.mark.parametrize("kernel", OC.DECODER_KERNELS, ids=OC.KERNEL_ID)
@pytest.mark.parametrize("path", [(0,), (1,)], ids=["sigma", "rgb"])
@pytest.mark.parametrize("P,B", OC.DECODER_SHAPES)
def test_decoder_each_path_alone_against_float64(amd, dev, oracle_params, P, B, path, kernel):
    ops = amd.ops
    cpu, args, masks, up = decoder_launch(amd, dev, oracle_params, P, B, kernel[0])
    got, _ = decoder_bwd(ops, args, OC.keep(up, path), kernel)
    wts = OC.keep(cpu[3], path, torch.zeros_like)
    r32, r64 = [OC.oracle_decoder(oracle_params, *cpu[:3], masks, wts, dt) for dt in (torch.float32, torch.float64)]
    OC.hold_decoder_path(f"decoder {P}/{B} {OC.KERNEL_ID(kernel)} {'sigma' if path == (0,) else 'rgb'}-only", got, r32, r64, band_of(kernel[0]),
                         reaches_colour=path == (1,))


def test_decoder_sigma_only_with_null_rgb_is_the_density_backward(amd, dev, oracle_params):
    """fp32, 64-point objects (``density_bwd``'s latent gradient needs them): d_xyz and the shape rows, bit for bit; the texture rows zero."""
    ops = amd.ops
    P, B = OC.DENSITY_SHAPE
    _, args, _, up = decoder_launch(amd, dev, oracle_params, P, B, "fp32")
    xyz, _, lat, packed, mk, sig = args
    full, _ = decoder_bwd(ops, args, (up[0], None), ("fp32", False))
    with OC.nan_filled_outputs(ops):
        d_lat, d_xyz = ops.density_bwd(xyz, lat, packed, mk, sig, up[0], SB, TB)
    assert OC.written(d_lat) and OC.written(d_xyz) and float(d_xyz.abs().max()) > 0 and float(d_lat[:, :SB].abs().max()) > 0
    assert torch.equal(d_xyz, full["d_xyz"]) and torch.equal(d_lat[:, :SB], full["d_latent"][:, :SB])
    assert OC.zeros_equal(d_lat[:, SB:]) and OC.zeros_equal(full["d_latent"][:, SB:]) and OC.zeros_equal(full["d_dir"])


# ------------------------------------------------------------------ c. snr_density_bwd
def test_density_dropping_an_output_changes_no_other(amd, dev, oracle_params):
    """One kernel whatever is asked for: every comparison bit for bit."""
    ops = amd.ops
    P, B = OC.DENSITY_SHAPE
    cpu = OC.decoder_inputs(P, B)
    xyz, lat, d_sig = cpu[0].to(dev), cpu[2].to(dev), cpu[3][0].to(dev)
    packed = make_model(amd, dev, oracle_params, "fp32").packed_weights()
    sig, mk = ops.density_fwd(xyz, lat, packed, SB, TB, save_masks=True)
    got = {}
    for need_latent, need_xyz in ((True, True), (True, False), (False, True)):
        with OC.nan_filled_outputs(ops):
            got[need_latent, need_xyz] = dict(zip(("d_latent", "d_xyz"), ops.density_bwd(xyz, lat, packed, mk, sig, d_sig, SB, TB, need_latent=need_latent,
                                                                                        need_xyz=need_xyz)))
    assert got[True, False]["d_xyz"] is None and got[False, True]["d_latent"] is None
    same_bits("density latent alone", got[True, False], got[True, True], ["d_latent"])
    same_bits("density xyz alone", got[False, True], got[True, True], ["d_xyz"])
    assert float(got[True, True]["d_xyz"].abs().max()) > 0 and float(got[True, True]["d_latent"][:, :SB].abs().max()) > 0


# ------------------------------------------------------------------ d. snr_composite_bwd
COMPOSITE_OUTPUTS = ("d_sigma", "d_rgbs", "d_z")


def composite_bwd(ops, dev, operands, mode, white, up, need_dz):
    zmode = {"shared": ops.Z_SHARED, "per_ray": ops.Z_PER_RAY}[mode]
    with OC.nan_filled_outputs(ops):
        return dict(zip(COMPOSITE_OUTPUTS, ops.composite_bwd(*operands, zmode, white, 0, *up, need_dz)))


@pytest.mark.parametrize("case", OC.COMPOSITE_CASES, ids=OC.COMPOSITE_ID)
def test_composite_null_upstream_and_dropped_dz(amd, dev, case):
    ops = amd.ops
    S, mode, white = case
    sig, rgbs, zt, wts = OC.composite_inputs(S, mode)
    operands, up = [x.to(dev) for x in (sig, rgbs, zt)], tuple(w.to(dev) for w in wts)
    per_ray = mode == "per_ray"
    keys = COMPOSITE_OUTPUTS if per_ray else COMPOSITE_OUTPUTS[:2]
    for s in OC.SUBSETS:
        null = composite_bwd(ops, dev, operands, mode, white, OC.keep(up, s), per_ray)
        zero = composite_bwd(ops, dev, operands, mode, white, OC.keep(up, s, torch.zeros_like), per_ray)
        same_bits(f"composite {OC.COMPOSITE_ID(case)} upstream {OC.SUBSET_ID(s)}", null, zero, keys)
        assert float(null["d_sigma"].abs().max()) > 0
        if per_ray:                                                   # contract 2: d_z dropped
            lean = composite_bwd(ops, dev, operands, mode, white, OC.keep(up, s), False)
            assert lean["d_z"] is None
            same_bits(f"composite {OC.COMPOSITE_ID(case)} without d_z", lean, null, COMPOSITE_OUTPUTS[:2])
    nothing = composite_bwd(ops, dev, operands, mode, white, (None, None, None), per_ray)
    for k in keys:
        assert OC.written(nothing[k]) and OC.zeros_equal(nothing[k]), k


@pytest.mark.parametrize("path", OC.SINGLES, ids=OC.SUBSET_ID)
@pytest.mark.parametrize("case", OC.COMPOSITE_CASES, ids=OC.COMPOSITE_ID)
def test_composite_each_path_alone_against_float64(amd, dev, case, path):
    ops = amd.ops
    S, mode, white = case
    sig, rgbs, zt, wts = OC.composite_inputs(S, mode)
    operands, up = [x.to(dev) for x in (sig, rgbs, zt)], tuple(w.to(dev) for w in wts)
    got = composite_bwd(ops, dev, operands, mode, white, OC.keep(up, path), mode == "per_ray")
    r32, r64 = OC.oracle_composite(sig, rgbs, zt, wts, mode, white, path)
    tag = f"composite {OC.COMPOSITE_ID(case)} {OC.SUBSET_ID(path)}-only"
    keys = [k for k in COMPOSITE_OUTPUTS if got[k] is not None]
    if path != (0,):                                                  # only the rgb output reads the colours
        assert OC.written(got["d_rgbs"]) and OC.zeros_equal(got["d_rgbs"]) and OC.zeros_equal(r64["d_rgbs"]), tag
        keys.remove("d_rgbs")
    assert all(float(r64[k].abs().max()) > 0 for k in keys)
    bad = [(r, k) for r, k in torch.nonzero((sig <= 0) & (got["d_sigma"].cpu() != 0)).tolist()]
    assert not bad, (tag, "d_sigma is not exactly 0.0 where sigma <= 0", bad[:8])
    check_all([(f"{tag} {k}", got[k], r32[k], r64[k]) for k in keys], "fp32")
    print(f"[optional operands] {tag}: worst {max(in_band(got[k], r32[k], r64[k], 'fp32')[1] for k in keys):.3f} of its band")


# ------------------------------------------------------------------ e. snr_scene_composite_bwd
@pytest.mark.parametrize("Nb,S,P", OC.SCENE_SHAPES)
def test_scene_composite_dropping_dz_changes_no_other(amd, dev, Nb, S, P):
    ops = amd.ops
    sig, rgb, z, wts = OC.scene_inputs(Nb, S, P)
    operands, up = [x.to(dev) for x in (sig, rgb, z)], tuple(w.to(dev) for w in wts)
    for run in (0, S):
        for s in ((0,), (0, 1, 2)):                                   # (d_rgb is required; NULL d_depth / d_acc: tests/test_scene_grad_gpu.py)
            with OC.nan_filled_outputs(ops):
                full = dict(zip(COMPOSITE_OUTPUTS, ops.scene_composite_bwd(*operands, True, run, *OC.keep(up, s), need_dz=True)))
                lean = dict(zip(COMPOSITE_OUTPUTS, ops.scene_composite_bwd(*operands, True, run, *OC.keep(up, s), need_dz=False)))
            assert lean["d_z"] is None and OC.written(full["d_z"]) and float(full["d_sigma"].abs().max()) > 0
            same_bits(f"scene ({Nb},{S},{P}) run {run} without d_z", lean, full, COMPOSITE_OUTPUTS[:2])
