"""Test helper: the optional operands of the five backward entry points -- launches, operand subsets, oracle calls, judgement.  CPU only
(the functions that launch take ``ops`` / the package as an argument; nothing here imports it).

include/supnerf_hip.h promises that an upstream gradient passed as NULL counts as zero and that every output may be NULL.  Three contracts
follow, and tests/test_optional_operands_gpu.py holds every entry point to them (tests/test_optional_operands_cpu.py shows on the oracle
alone that the third has teeth where the combined loss of the other render tests has few):

1. a NULL upstream gradient gives the bits of a zeros tensor in its place (the kernels substitute 0.f);
2. dropping an output changes no other output, bit for bit, whenever the same kernel runs.  Exact fp32 has two backward kernels, and
   ``snr_fp32_bwd16_supported_`` (csrc/snr_mlp16_bwd.hip) picks between them by, among others, whether latent partials are written:
   ``fp32_latent_toggle_changes_kernel`` restates that choice.  Outputs are therefore compared with the launch of the same ``need_latent``
   that requests everything else; the two such launches agree bit for bit where one kernel serves both and are held to the band otherwise;
3. each path alone -- exactly one upstream gradient not NULL -- is right against float64, mask-matched, in the project's bands; what a path
   cannot reach is exactly zero.

The render launches are the smallest that reach every branch of ``ray_grad_tail`` / ``ray_finish`` (csrc/snr_device.hpp) on the three
backward kernels, (3, 1) blocks, points per object 96 / 128 / 192 / 384 (whole 32-point tiles: the split kernels take all of them):

    ("shared", 8, 12, 2)     G = S < PW lanes share a ray; 96 points per object: fp32 runs the 16x16 kernel without d_latent and the
                             32x32 kernel with it; 192 points: the last 128-point workgroup of the 32x32 and split kernels is partial
    ("per_ray", 32, 4, 2)    d_t exists; S / PW = 2 on the 16x16 kernel (the LDS combine across waves); 128 points per object
    ("box", 64, 3, 2)        bounds' gradient through ray_finish, c[0..2] /= zs; S / PW = 4 on the 16x16 kernel; 4 rays hit, 2 miss
    ("per_object", 128, 3, 1)  fp32 always the 32x32 kernel, waves_per_ray = 4

Geometry, codes, latent terms and upstream weights are those of tests/render_geometry_cases.py (metric depths, white background, a frame
that is not the identity, distinct per-object scales), so the SNR_METRIC_Z term ``k`` of ``ray_grad_tail`` is live in every launch."""
import contextlib
import itertools

import torch
import torch.nn.functional as F

import render_geometry_cases as RG
import scene_grad_restatement as SR
import unfused_seam_cases as UC
from oracle import supnerf_oracle as O
from oracle_bands import check_all, check_per_object, check_per_ray, in_band, per_ray_errors

SB, TB = 3, 1
PATHS = ("rgb", "depth", "acc")
# every non-empty subset of the three upstream gradients, as indices into PATHS; the three single ones first
SUBSETS = [s for k in (1, 2, 3) for s in itertools.combinations(range(3), k)]
SINGLES = SUBSETS[:3]
SUBSET_ID = lambda s: "+".join(PATHS[i] for i in s)

RENDER_LAUNCHES = [("shared", 8, 12, 2), ("per_ray", 32, 4, 2), ("box", 64, 3, 2), ("per_object", 128, 3, 1)]
LAUNCH_ID = lambda c: f"{c[0]}-S{c[1]}-n{c[2]}-B{c[3]}"
RENDER_OUTPUTS = ("d_rays_o", "d_rays_d", "d_t", "d_latent")
PLANT = 1.0 + 2.0 ** -7          # the planted error: 0.8 %, above every floor of BANDS and the 1e-3 of the per-ray rule, far below a wrong formula


def fp32_latent_toggle_changes_kernel(points_per_obj, S=None, layer_grads=False):
    """``snr_fp32_bwd16_supported_`` restated: does an exact-fp32 launch move between the 16x16 and the 32x32 kernel when d_latent is
    toggled?  Training dumps (``layer_grads``) and, in render mode, a ray longer than 64 samples take the 32x32 kernel either way; otherwise
    the 16x16 kernel runs unless latent partials are wanted for objects that are no multiple of 64 points."""
    if layer_grads or (S is not None and not (S <= 64 and 64 % S == 0)):
        return False
    return points_per_obj % 64 != 0


def keep(values, subset, other=None):
    """``values`` with the entries outside ``subset`` replaced: None (a NULL pointer), or ``other(value)``."""
    return tuple(v if i in subset else (None if other is None else other(v)) for i, v in enumerate(values))


def zeros_equal(x):
    return bool((x == 0).all())           # (zeros of either sign)


def written(x):
    return bool(torch.isfinite(x).all())


class _NanEmpty:
    """``torch`` as ``ops`` sees it inside ``nan_filled_outputs``: ``empty`` / ``empty_like`` hand out NaN instead of whatever the allocator
    held (most likely the previous launch's result of the same shape, which would pass for a written output)."""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        return getattr(self._real, name)

    @staticmethod
    def _fill(t):
        return t.fill_(float("nan")) if t.is_floating_point() else t

    def empty(self, *a, **k):
        return self._fill(self._real.empty(*a, **k))

    def empty_like(self, *a, **k):
        return self._fill(self._real.empty_like(*a, **k))


@contextlib.contextmanager
def nan_filled_outputs(ops):
    """Every float buffer an operator of ``ops`` allocates for the C ABI inside the block starts as NaN: an element the kernel does not
    write stays NaN and fails ``written``."""
    real = ops.torch
    ops.torch = _NanEmpty(real)
    try:
        yield
    finally:
        ops.torch = real


# ------------------------------------------------------------------ a. the fused render
def render_cfg(ops, c, dev, precision):
    zmode = {"shared": ops.Z_SHARED, "per_object": ops.Z_PER_OBJECT, "per_ray": ops.Z_PER_RAY, "box": ops.Z_BOX}[c.mode]
    return ops.RenderCfg(c.S, zmode, c.n, SB, TB, frame=tuple(c.frame.flatten().tolist()), xyz_mul=c.xyz_mul, white_bkgd=True, metric_z=True,
                         precision=precision, box_half=c.box_half.to(dev) if c.mode == "box" else None)


def render_output_subsets(c):
    """name -> need_* flags of ``ops.render_bwd``: everything, each output dropped alone, each of o / d / t kept alone, and d_t with the
    latent gradient but neither ray output (the early return of ``ray_grad_tail`` in front of a live reduction)."""
    per_ray = c.mode == "per_ray"
    full = dict(need_o=True, need_d=True, need_t=per_ray, need_latent=True)
    none = dict.fromkeys(full, False)
    subs = {"full": full}
    subs.update({"no_" + k: {**full, k: False} for k, v in full.items() if v})
    subs.update({"only_" + k: {**none, k: True} for k in ("need_o", "need_d")})
    if per_ray:
        subs["only_need_t"] = {**none, "need_t": True}
        subs["need_t_and_latent"] = {**none, "need_t": True, "need_latent": True}
    return subs


def single_path(c, subset):
    """The launch whose oracle loss reads the outputs of ``subset`` alone (the other weights are zeros: they multiply out exactly)."""
    return c._replace(wts=keep(c.wts, subset, torch.zeros_like))


def oracle_relu_pattern(params, c):
    """The ReLU pattern of the launch in float64 (no GPU at hand): one bool (N,S,width) tensor per ReLU layer, forward order."""
    p = {k: v.double() for k, v in params.items()}
    pts, _ = RG.decoder_frame_points(c)
    dirs = (c.rays_d.double() @ c.frame.double().T)[:, None, :].expand_as(pts)
    rec = []
    with torch.no_grad():
        O.decoder_forward(p, pts, dirs, None, None, latent=c.latent.double(), taps=rec)
    return [out > 0 for name, _, out in rec if name not in ("encoding_shape", "sigma.0", "rgb.2")]


def ray_rule_ratio(got, o32, o64):
    """The worst ray's error over what ``check_per_ray`` allows it: max(1e-3, 8 x the fp32 oracle's error on that ray)."""
    err, floor = per_ray_errors(got, o32, o64)
    return float((err / torch.maximum(torch.full_like(floor, 1e-3), 8 * floor)).max())


def object_band_ratio(got, o32, o64, band):
    """The worst object's error over its band (``check_per_object``); inf when an object is outside."""
    return max(in_band(got[b], o32[b], o64[b], band)[1] for b in range(o64.shape[0]))


def hold_render_path(tag, got, r32, r64, band, reaches_texture, per_object=("d_latent",)):
    """Contract 3 on the gradients of a render launch: every ray by the per-ray rule, every object's rows in ``band``, every float64
    gradient held to either not identically zero; the texture rows (and the texture code's gradient) exactly zero where the loss cannot
    reach them.  Returns the worst (tensor, ray) ratios."""
    bad, worst_ray, worst_obj = [], 0.0, 0.0
    for k in ("d_rays_o", "d_rays_d", "d_t"):
        assert (got[k] is None) == (r64[k] is None), k
        if got[k] is None:
            continue
        assert float(r64[k].abs().max()) > 0, f"{tag} {k}: the float64 gradient is identically zero"
        bad += check_per_ray(f"{tag} {k}", got[k], r32[k], r64[k])
        worst_ray = max(worst_ray, ray_rule_ratio(got[k], r32[k], r64[k]))
    assert not bad, bad
    pairs = []
    for k in per_object:
        g, a, b = [x.detach().cpu() for x in (got[k], r32[k], r64[k])]
        if not reaches_texture:
            if k == "d_texturecode":
                assert zeros_equal(g) and zeros_equal(b), f"{tag} {k}: a loss without rgb reached the texture code"
                continue
            if k == "d_latent":
                assert zeros_equal(g[:, SB:]) and zeros_equal(b[:, SB:]), f"{tag} {k}: a loss without rgb reached the texture rows"
                g, a, b = g[:, :SB], a[:, :SB], b[:, :SB]
        assert bool((b.flatten(1).abs().amax(1) > 0).all()), f"{tag} {k}: an object's float64 gradient is identically zero"
        pairs.append((f"{tag} {k}", g, a, b))
        worst_obj = max(worst_obj, object_band_ratio(g, a, b, band))
    check_per_object(pairs, band)
    print(f"[optional operands] {tag}: worst object {worst_obj:.3f} of its band, worst ray {worst_ray:.3f} of the per-ray rule")
    return worst_obj, worst_ray


# ------------------------------------------------------------------ b., c. the decoder on points
DECODER_SHAPES = [(192, 2), (96, 3)]                 # (P, B): 96 and 32 points per object -- never a multiple of 64
DECODER_KERNELS = [("fp32", False), ("fp32", True), ("bf16x3", False)]       # (precision, layer_grads): 16x16 | 32x32, 32x32, split
KERNEL_ID = lambda k: k[0] + ("-layer_grads" if k[1] else "")
DECODER_OUTPUTS = ("d_latent", "d_xyz", "d_dir")
DENSITY_SHAPE = (128, 2)                             # 64-point objects: what density_bwd's latent gradient needs


def decoder_inputs(P, B, seed=0):
    """xyz (P,3) in the unit cube, unit viewdir (P,3), latent terms (B,4,256) distinct per object, upstream weights of sigma (P,) and rgb (P,3)."""
    g = torch.Generator().manual_seed(4000 + P + 7 * B + seed)
    xyz = torch.rand(P, 3, generator=g) * 2 - 1
    vd = F.normalize(torch.randn(P, 3, generator=g), dim=-1)
    lat = torch.relu(torch.randn(B, SB + TB, 256, generator=g) * 0.3)
    return xyz, vd, lat, (torch.randn(P, generator=g), torch.randn(P, 3, generator=g))


def decoder_output_subsets():
    names = ("need_latent", "need_xyz", "need_dir")
    subs = {"full": dict.fromkeys(names, True)}
    subs.update({"no_" + k: {**subs["full"], k: False} for k in names})
    subs.update({"only_" + k: {**dict.fromkeys(names, False), k: True} for k in names})
    return subs


def oracle_decoder(params, xyz, vd, lat, masks, wts, dt):
    """Gradients of sum(sigma w_s) + sum(rgb w_r) on the oracle in ``dt``: dict over DECODER_OUTPUTS."""
    p = {k: v.to(dt) for k, v in params.items()}
    x, v, l = [t.to(dt).clone().requires_grad_() for t in (xyz, vd, lat)]
    s, r = O.decoder_forward(p, x[:, None], v[:, None], None, None, relu_masks=masks, latent=l)
    ((s.reshape(-1) * wts[0].to(dt)).sum() + (r.reshape(-1, 3) * wts[1].to(dt)).sum()).backward()
    return dict(d_latent=l.grad, d_xyz=x.grad, d_dir=v.grad)


def hold_decoder_path(tag, got, r32, r64, band, reaches_colour):
    """Contract 3 on ``snr_decoder_bwd``: d_xyz, d_dir in the tensor band, every object's latent rows in it; a sigma-only loss leaves
    d_viewdir and the texture rows exactly zero."""
    tensors, lat = ["d_xyz"], [x.detach().cpu() for x in (got["d_latent"], r32["d_latent"], r64["d_latent"])]
    if reaches_colour:
        tensors.append("d_dir")
    else:
        assert zeros_equal(got["d_dir"]) and zeros_equal(r64["d_dir"]), f"{tag}: a sigma-only loss reached d_viewdir"
        assert zeros_equal(lat[0][:, SB:]) and zeros_equal(lat[2][:, SB:]), f"{tag}: a sigma-only loss reached the texture rows"
        lat = [x[:, :SB] for x in lat]
    for k in tensors:
        assert float(r64[k].abs().max()) > 0, (tag, k)
    assert bool((lat[2].flatten(1).abs().amax(1) > 0).all()), tag
    check_all([(f"{tag} {k}", got[k], r32[k], r64[k]) for k in tensors], band)
    check_per_object([(f"{tag} d_latent", *lat)], band)
    worst = max([in_band(got[k], r32[k], r64[k], band)[1] for k in tensors] + [object_band_ratio(*lat, band)])
    print(f"[optional operands] {tag}: worst {worst:.3f} of its band")
    return worst


# ------------------------------------------------------------------ d. the stand-alone composite
COMPOSITE_N = 7
COMPOSITE_CASES = [(S, mode, white) for S in (5, 64, 65) for mode in ("shared", "per_ray") for white in (True, False)]
COMPOSITE_ID = lambda c: f"S{c[0]}-{c[1]}-{'white' if c[2] else 'black'}"


def composite_inputs(S, mode):
    """sigma (N,S), rgbs (N,S,3), the depth table of ``mode``, upstream weights: ``unfused_seam_cases.seam_inputs``."""
    sig, rgbs, z, wts = UC.seam_inputs(COMPOSITE_N, S, seed=900 + S)
    return sig, rgbs, UC.depth_table(z, mode), tuple(wts)


def oracle_composite(sig, rgbs, zt, wts, mode, white, subset):
    """(fp32, float64) references of the loss that reads the outputs of ``subset`` alone: dicts with d_sigma, d_rgbs, d_z."""
    return UC.references(sig, rgbs, zt, list(keep(wts, subset, torch.zeros_like)), mode, 0, white)


# ------------------------------------------------------------------ e. the scene composite
SCENE_SHAPES = [(3, 5, 9), (2, 32, 7)]               # (objects, samples, pixels): n = 15 and n = 64 samples per pixel


def scene_inputs(Nb, S, P):
    sig, rgb, z = SR.shape_case(Nb, S, P)
    g = torch.Generator().manual_seed(Nb + S + P)
    return sig, rgb, z, (torch.randn(P, 3, generator=g), torch.randn(P, generator=g), torch.randn(P, generator=g))
