"""Test helper: inputs, float64 / fp32 reference and judgement for the stand-alone composite at its seams.  CPU only.

``snr_composite_fwd`` (csrc/snr_aux.hip) takes ``composite_fwd16_kernel`` -- 16 lanes per ray, four consecutive samples per lane, four
rays per wave -- for S <= 64, S % 4 == 0 and 16-byte aligned operands, ``composite_fwd_kernel`` (one wave per ray) otherwise;
``snr_composite_bwd`` always runs one wave per ray.  All three walk the rays with a grid-stride loop.  The seams: a row of lanes that S
does not fill, a group of four rays that the ray count does not fill or that an object boundary cuts, the second trip of the loop, and
densities <= 0 (no gradient).  tests/test_unfused_seams_gpu.py runs the kernels on these inputs and judges them with the functions below;
tests/test_unfused_seams_cpu.py feeds the same functions torch restatements of kernels that are wrong at one seam each (``restated``) and
holds them to noticing."""
import torch

from oracle import supnerf_oracle as O
from oracle_bands import check_all, in_band

OUTPUTS = ("rgb", "depth", "acc")
NAMES = OUTPUTS + ("d_sigma", "d_rgbs", "d_z")
WRONG = ("last_interval_at_lane_15", "group_takes_its_first_rays_object", "ray_dropped", "negative_density_gradient", "trip_not_written",
         "trip_repeats_the_first")


def seam_inputs(N, S, seed):
    """sigma (N,S) in -0.5 .. 2.5 -- about one in six negative -- with a tenth exactly 0.0, rgbs (N,S,3) normal, z (N,S) ascending in 4 .. 7,
    upstream weights for rgb (N,3), depth (N) and acc (N): fp32."""
    g = torch.Generator().manual_seed(seed)
    sig = torch.rand(N, S, generator=g) * 3 - 0.5
    sig[torch.rand(N, S, generator=g) < 0.1] = 0.0
    rgbs = torch.randn(N, S, 3, generator=g)
    z = torch.sort(torch.rand(N, S, generator=g) * 3 + 4, dim=-1)[0]
    wts = [torch.randn(N, 3, generator=g), torch.randn(N, generator=g), torch.randn(N, generator=g)]
    return sig, rgbs, z, wts


def depth_table(z, mode, rays_per_obj=0):
    """The operand ``z_vals`` of a depth layout, cut from per-ray depths (N,S): row 0 (shared), every object's first ray's row (per object:
    the rows of different objects differ), or all of it."""
    return {"shared": lambda: z[0], "per_object": lambda: z[::max(rays_per_obj, 1)], "per_ray": lambda: z}[mode]().contiguous()


def depth_rows(zt, mode, N, rays_per_obj=0):
    """The (N,S) depths a table means."""
    return {"shared": lambda: zt[None].expand(N, -1), "per_object": lambda: zt.repeat_interleave(max(rays_per_obj, 1), 0), "per_ray": lambda: zt}[mode]()


def composite(sig, rgbs, z, white, last_delta=None, relu=torch.relu):
    """``oracle.composite`` with the width of the last interval and the clamp of the density open to a restatement of a wrong kernel."""
    delta = torch.cat([z[..., 1:] - z[..., :-1], torch.full_like(z[..., :1], O.LAST_DELTA) if last_delta is None else last_delta], dim=-1)
    alpha = 1 - torch.exp(-relu(sig) * delta)
    trans = 1 - alpha + O.TRANS_EPS
    acc = torch.cumprod(torch.cat([torch.ones_like(trans[..., :1]), trans], dim=-1), dim=-1)[..., :-1]
    w = alpha * acc
    rgb = (w[..., None] * rgbs).sum(-2)
    if white:
        rgb = rgb + 1 - w.sum(-1)[..., None]
    return rgb, (w * z).sum(-1), acc[..., -1]


def reference(sig, rgbs, zt, wts, mode, rays_per_obj, white, dt, backward=True, fn=None):
    """Outputs and gradients of sum_i (out_i * w_i) on the oracle in ``dt``: a dict over ``NAMES``; d_z for per-ray depths only, no gradients
    with ``backward`` off.  ``fn(s, r, z_rows, white)`` replaces ``oracle.composite``."""
    N = sig.shape[0]
    s, r, zz = [x.to(dt).clone().requires_grad_(backward) for x in (sig, rgbs, zt)]
    out = (fn or (lambda a, b, c, w: O.composite(a, b, c, white_bkgd=w)))(s, r, depth_rows(zz, mode, N, rays_per_obj), white)
    res = {k: v.detach() for k, v in zip(OUTPUTS, out)}
    if backward:
        sum((a * w.to(dt)).sum() for a, w in zip(out, wts)).backward()
        res.update(d_sigma=s.grad, d_rgbs=r.grad, d_z=zz.grad if mode == "per_ray" else None)
    return res


def references(sig, rgbs, zt, wts, mode, rays_per_obj, white, backward=True):
    """(fp32 oracle: the noise sample, float64 oracle: the value)."""
    return [reference(sig, rgbs, zt, wts, mode, rays_per_obj, white, dt, backward) for dt in (torch.float32, torch.float64)]


# ------------------------------------------------------------------ judgement
def zero_gradient_violations(d_sigma, sig):
    """Samples with sigma <= 0 whose d_sigma is not exactly 0.0 (``composite_ray_bwd``: ``sig > 0``), as (ray, sample) pairs."""
    return torch.nonzero((sig.cpu() <= 0) & (d_sigma.detach().cpu() != 0)).tolist()


def judge(tag, got, r32, r64, sig):
    """Every tensor of ``got`` (a dict over ``NAMES``; a forward-only or backward-only result holds its half alone) in the fp32 band of
    ``oracle_bands.check_all`` -- which a value that is not finite, i.e. was never written over its NaN fill, leaves -- and d_sigma exactly
    0.0 wherever sigma <= 0.  Returns the largest error-to-band ratio."""
    keys = [k for k in NAMES if k in got and r64.get(k) is not None]
    assert set(OUTPUTS) <= set(keys) or {"d_sigma", "d_rgbs"} <= set(keys), keys
    assert all(got[k] is not None for k in keys) and all(got[k] is None for k in got if k not in keys), (tag, keys, list(got))
    pairs = [(f"{tag} {k}", got[k].reshape(r64[k].shape), r32[k], r64[k]) for k in keys]
    check_all(pairs, "fp32")
    if "d_sigma" in got:
        bad = zero_gradient_violations(got["d_sigma"].reshape(sig.shape), sig)
        assert not bad, (tag, "d_sigma is not exactly 0.0 where sigma <= 0 at (ray, sample)", bad[:8])
    return max(in_band(g, a, b, "fp32", n)[1] for n, g, a, b in pairs)


def position_mismatches(base, moved, perm):
    """``moved`` is the result on the rays ``perm`` of ``base``'s launch, i.e. ray perm[i] stood in slot i.  A ray's arithmetic may not
    depend on its slot in the group of four or in the wave: the names of the tensors whose rows are not the same bits."""
    return [k for k in NAMES if base.get(k) is not None and not torch.equal(moved[k].cpu(), base[k].cpu()[perm])]


def trip_mismatches(got, head, first):
    """The rays ``first`` .. of a launch (the later trips of its grid-stride loop) against ``head``, the same ray data at the head of a small
    launch: the names of the tensors whose rows are not the same bits."""
    return [k for k in NAMES if head.get(k) is not None and not torch.equal(got[k].reshape(-1, *head[k].shape[1:])[first:].cpu(), head[k].cpu())]


# ------------------------------------------------------------------ restatements, right and wrong
def restated(sig, rgbs, zt, wts, mode, rays_per_obj, white, wrong=None, sweep=None, dropped=None, backward=True):
    """What a kernel gives, restated in torch on the fp32 oracle: a dict over ``NAMES``.  ``wrong`` is None (the kernel as it should be)
    or one mistake of ``WRONG``:

    last_interval_at_lane_15           the 1e10 interval is applied at sample 63, the row's last, not at S - 1: sample S - 1 of a shorter ray
                                       gets delta = 0 - z, the idle next lane's depth minus its own
    group_takes_its_first_rays_object  the four rays of a group read the depth row of the object of the group's first ray
    ray_dropped                        ray ``dropped`` is never written: zeros, what a fresh ``torch.empty`` block tends to hold
    negative_density_gradient          d_sigma is not zeroed where sigma <= 0
    trip_not_written                   the rays past the first ``sweep`` are left as the caller's NaN fill
    trip_repeats_the_first             ray sweep + i is given the results of ray i"""
    assert wrong is None or wrong in WRONG, wrong
    N, S = sig.shape
    fn, z_mode, table = None, mode, zt
    if wrong == "last_interval_at_lane_15" and S < 64:
        fn = lambda s, r, z, w: composite(s, r, z, w, last_delta=0 - z[..., -1:])
    if wrong == "negative_density_gradient":
        fn = lambda s, r, z, w: composite(s, r, z, w, relu=lambda x: x + (torch.relu(x) - x).detach())
    if wrong == "group_takes_its_first_rays_object" and mode == "per_object":
        ray = torch.arange(N)
        table, z_mode = zt[(ray // 4 * 4) // rays_per_obj], "per_ray"
    res = reference(sig, rgbs, table, wts, z_mode, rays_per_obj, white, torch.float32, backward, fn)
    if mode != "per_ray":
        res["d_z"] = None
    if not backward:
        res = {k: res[k] for k in OUTPUTS}
    for k, v in res.items():
        if v is None:
            continue
        if wrong == "ray_dropped":
            v[dropped] = 0.0
        if wrong == "trip_not_written":
            v[sweep:] = float("nan")
        if wrong == "trip_repeats_the_first":
            v[sweep:] = v[: N - sweep].clone()
    return res
