"""The single-path checks of tests/test_optional_operands_gpu.py on the oracle alone: how much of the combined loss's gradient each
upstream path is, and whether a path that is 0.8 % wrong (``optional_operand_cases.PLANT`` = 1 + 2^-7) is noticed.  No GPU.

The render tests elsewhere send sum(rgb w) + sum(depth w) + sum(acc w) with normal weights through the backward and judge the sum.  Here
the float64 oracle (raw route: given latent terms; its own ReLU pattern imposed on the fp32 run, as the GPU tests impose the kernel's)
differentiates the three single-path losses and their sum on every launch of ``optional_operand_cases.RENDER_LAUNCHES``.

Measured shares, max |g_path| / max |g_sum| per output tensor (rgb / depth / acc):

    launch                 d_rays_o                d_rays_d                d_t                     d_latent
    shared-S8-n12-B2       0.676 / 0.972 / 0.514   0.096 / 0.978 / 0.150   -                       1.000 / 0.622 / 0.183
    per_ray-S32-n4-B2      0.734 / 0.775 / 0.905   0.031 / 0.998 / 0.105   0.047 / 0.987 / 0.144   1.000 / 0.482 / 0.129
    box-S64-n3-B2          0.037 / 1.003 / 0.005   0.151 / 1.025 / 0.045   -                       1.000 / 0.113 / 0.094
    per_object-S128-n3-B1  0.831 / 0.749 / 0.152   0.050 / 0.997 / 0.039   -                       0.757 / 1.217 / 0.189

So with unit-normal weights on metric depths the depth path is no small term: it IS the direction's and the per-ray depths' gradient (the
rgb path is 3 .. 15 % of it there) and, through the box bounds, the origin's; rgb leads only in d_latent.  The small one is acc: 0.5 % of
d_rays_o and 4.5 % of d_rays_d under box sampling, 4 % of d_rays_d with 128 samples, 10 .. 19 % of d_latent.

What the planted error does.  Alone, every path's own check rejects it on every tensor it reaches: every ray gradient by the per-ray rule,
the latent rows in the fp32 and in the bf16x3 band (asserted below).  Added to the combined gradient and judged as the other render tests
judge the sum (reported, not asserted): a wrong depth path is rejected on every tensor of every launch; a wrong acc path is ACCEPTED on
d_rays_o and d_rays_d of box-S64-n3-B2 and on d_rays_d of per_object-S128-n3-B1, and rejected elsewhere.  The combined loss does hide the
acc path from the ray gradients where that path is a few percent of the sum; it does not hide the depth path.
"""
import types

import pytest
import torch

import optional_operand_cases as OC
import render_geometry_cases as RG
from oracle_bands import BANDS, check_per_ray, in_band

ALL = OC.SUBSETS[-1]
_RUNS = {}


def oracle_runs(params, case):
    """The launch, and per subset of SINGLES + (all three) the (fp32, float64) oracle gradients on the float64 ReLU pattern."""
    if case not in _RUNS:
        c = RG.build(case)
        masks = OC.oracle_relu_pattern(params, c)
        _RUNS[case] = c, {s: [RG.oracle(params, OC.single_path(c, s), dt, masks=masks, latent=c.latent) for dt in (torch.float32, torch.float64)]
                          for s in OC.SINGLES + [ALL]}
    return _RUNS[case]


def outputs_of(r):
    return [k for k in OC.RENDER_OUTPUTS if r[k] is not None]


def rays_accept(name, got, o32, o64):
    return not check_per_ray(name, got, o32, o64)


def objects_accept(got, o32, o64, band):
    return all(in_band(got[b], o32[b], o64[b], band)[0] for b in range(o64.shape[0]))


# ------------------------------------------------------------------ the lists
def test_the_lists_are_what_the_kernels_need():
    assert len(OC.SUBSETS) == 7 and OC.SINGLES == [(0,), (1,), (2,)] and ALL == (0, 1, 2)
    assert OC.RENDER_LAUNCHES == [("shared", 8, 12, 2), ("per_ray", 32, 4, 2), ("box", 64, 3, 2), ("per_object", 128, 3, 1)]
    assert not set(OC.RENDER_LAUNCHES) & {r[1] for r in RG.RUNS}          # (local to these modules: RG.RUNS feeds other tests)
    for mode, S, n, B in OC.RENDER_LAUNCHES:
        assert S * n * B <= 384 and (S * n) % 32 == 0                       # small, and whole wave tiles: no padding, the split kernels run
    # which exact-fp32 kernel: 96 points per object move between the two with d_latent, the others do not
    assert [OC.fp32_latent_toggle_changes_kernel(S * n, S) for _, S, n, _ in OC.RENDER_LAUNCHES] == [True, False, False, False]
    assert all(OC.fp32_latent_toggle_changes_kernel(P // B) and not OC.fp32_latent_toggle_changes_kernel(P // B, layer_grads=True)
               for P, B in OC.DECODER_SHAPES)
    assert not OC.fp32_latent_toggle_changes_kernel(OC.DENSITY_SHAPE[0] // OC.DENSITY_SHAPE[1])
    # the box launch: at least half of the rays hit, at least one misses
    c = RG.build(("box", 64, 3, 2))
    _, hit = RG.decoder_frame_points(c)
    assert 2 * int(hit.sum()) >= hit.numel() and not bool(hit.all()), hit.tolist()


def test_output_subsets():
    for case in OC.RENDER_LAUNCHES:
        c = RG.build(case)
        subs = OC.render_output_subsets(c)
        per_ray = c.mode == "per_ray"
        assert len(subs) == (9 if per_ray else 6) and all(any(f.values()) for f in subs.values())
        assert all(f["need_t"] is False for f in subs.values()) or per_ray
        if per_ray:
            assert subs["only_need_t"] == dict(need_o=False, need_d=False, need_t=True, need_latent=False)
    subs = OC.decoder_output_subsets()
    assert len(subs) == 7 and len({tuple(f.values()) for f in subs.values()}) == 7


def test_nan_filled_outputs_poisons_and_restores():
    ops = types.SimpleNamespace(torch=torch)
    with OC.nan_filled_outputs(ops):
        a, b, ws = ops.torch.empty(3, 2), ops.torch.empty_like(torch.zeros(4)), ops.torch.empty(8, dtype=torch.uint8)
        assert bool(torch.isnan(a).all()) and bool(torch.isnan(b).all()) and ws.dtype == torch.uint8
        assert ops.torch.zeros(2).tolist() == [0.0, 0.0]
    assert ops.torch is torch and not OC.written(a) and OC.written(torch.zeros(2))


# ------------------------------------------------------------------ shares of the sum
@pytest.mark.parametrize("case", OC.RENDER_LAUNCHES, ids=OC.LAUNCH_ID)
def test_single_paths_add_up_and_their_shares(oracle_params, case):
    c, runs = oracle_runs(oracle_params, case)
    total = runs[ALL][1]
    row = []
    for k in outputs_of(total):
        parts = [runs[s][1][k] for s in OC.SINGLES]
        top = float(total[k].abs().max())
        assert top > 0 and all(float(p.abs().max()) > 0 for p in parts), k
        # the loss is a sum of three: so is its float64 gradient, up to the order of the additions
        assert float((sum(parts) - total[k]).abs().max()) <= 1e-12 * top, k
        row.append(" / ".join(f"{float(p.abs().max()) / top:.3f}" for p in parts))
    print(f"[shares] {OC.LAUNCH_ID(case):22s} " + "   ".join(row) + "    (" + ", ".join(outputs_of(total)) + ")")


# ------------------------------------------------------------------ the planted error
@pytest.mark.parametrize("path", [1, 2], ids=lambda i: OC.PATHS[i])
@pytest.mark.parametrize("case", OC.RENDER_LAUNCHES, ids=OC.LAUNCH_ID)
def test_single_path_check_rejects_a_planted_error(oracle_params, case, path):
    c, runs = oracle_runs(oracle_params, case)
    (p32, p64), (s32, s64) = runs[(path,)], runs[ALL]
    report = []
    for k in outputs_of(p64):
        rows = slice(0, OC.SB) if k == "d_latent" else slice(None)          # (the texture rows of this path are zero: nothing to scale)
        cut = (lambda x: x[:, rows]) if k == "d_latent" else (lambda x: x)
        g32, g64, t32, t64 = [cut(x) for x in (p32[k], p64[k], s32[k], s64[k])]
        wrong_single, wrong_sum = g64 * OC.PLANT, t64 + g64 * (OC.PLANT - 1)
        if k == "d_latent":
            for band in BANDS:
                assert objects_accept(g64, g32, g64, band), (k, band)                         # (the right gradient is inside)
                assert not objects_accept(wrong_single, g32, g64, band), f"{k} [{band}]: the single-path check accepts the planted error"
            seen = {band: not objects_accept(wrong_sum, t32, t64, band) for band in BANDS}
        else:
            assert rays_accept(k, g64, g32, g64)
            assert not rays_accept(f"{k} planted", wrong_single, g32, g64), f"{k}: the single-path check accepts the planted error"
            seen = {"per-ray": not rays_accept(f"{k} planted in the sum", wrong_sum, t32, t64)}
        report.append(f"{k} " + ", ".join(f"{b}: {'rejected' if v else 'ACCEPTED'}" for b, v in seen.items()))
    print(f"[plant] {OC.LAUNCH_ID(case):22s} {OC.PATHS[path]:5s} SINGLE rejected everywhere; SUM " + "; ".join(report))


# ------------------------------------------------------------------ what a path cannot reach
@pytest.mark.parametrize("case", OC.RENDER_LAUNCHES, ids=OC.LAUNCH_ID)
def test_depth_and_acc_do_not_reach_the_texture_rows(oracle_params, case):
    c, runs = oracle_runs(oracle_params, case)
    for path in (1, 2):
        for r in runs[(path,)]:
            assert OC.zeros_equal(r["d_latent"][:, OC.SB:]) and float(r["d_latent"][:, :OC.SB].abs().max()) > 0
    assert float(runs[(0,)][1]["d_latent"][:, OC.SB:].abs().max()) > 0


@pytest.mark.parametrize("P,B", OC.DECODER_SHAPES + [OC.DENSITY_SHAPE])
def test_sigma_does_not_reach_viewdir_or_the_texture_rows(oracle_params, P, B):
    xyz, vd, lat, wts = OC.decoder_inputs(P, B)
    for dt in (torch.float32, torch.float64):
        r = OC.oracle_decoder(oracle_params, xyz, vd, lat, None, OC.keep(wts, (0,), torch.zeros_like), dt)
        assert OC.zeros_equal(r["d_dir"]) and OC.zeros_equal(r["d_latent"][:, OC.SB:])
        assert float(r["d_xyz"].abs().max()) > 0 and float(r["d_latent"][:, :OC.SB].abs().max()) > 0
        r = OC.oracle_decoder(oracle_params, xyz, vd, lat, None, OC.keep(wts, (1,), torch.zeros_like), dt)
        assert all(float(r[k].abs().max()) > 0 for k in OC.DECODER_OUTPUTS) and float(r["d_latent"][:, OC.SB:].abs().max()) > 0


@pytest.mark.parametrize("case", OC.COMPOSITE_CASES, ids=OC.COMPOSITE_ID)
def test_composite_depth_and_acc_do_not_reach_the_colours(case):
    S, mode, white = case
    sig, rgbs, zt, wts = OC.composite_inputs(S, mode)
    for subset in OC.SINGLES:
        for r in OC.oracle_composite(sig, rgbs, zt, wts, mode, white, subset):
            assert float(r["d_sigma"].abs().max()) > 0 and (mode != "per_ray" or float(r["d_z"].abs().max()) > 0)
            assert OC.zeros_equal(r["d_rgbs"]) == (subset != (0,))
