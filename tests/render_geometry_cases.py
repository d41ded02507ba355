"""Test helper: fused-render launches whose ray geometry is not the identity, and their oracle.  CPU only.

The render kernels place a sample of ray r, object b = r // rays_per_obj, at (csrc/snr_device.hpp ``make_sample``)

    p = M (((o + t d) / xyz_div[b]) * xyz_mul),   dir = M d,   zc = |t d| z_scale[b]

(SNR_Z_BOX: o = rays_o / z_scale[b], t from the slab test against +-box_half[b], xyz_div not applied) and take the gradient back through
``ray_grad_tail`` / ``ray_finish``: xyz_mul / xyz_div[b], M^T, 1 / z_scale[b].  The two-waves fp32 kernels derive b per lane by hand
(csrc/snr_mlp16_core.hpp ``point_id``).  Here every one of these parameters is something else than 1 / the identity and differs
between the objects of a launch, so that a wrong object index, a transposed frame or a dropped factor moves the numbers
(tests/test_render_geometry_cpu.py holds the cases to that; tests/test_render_geometry_gpu.py runs them on the kernels).

The rays are built backwards, in float64: decoder-frame rays (o', d', t') where the other render tests put theirs -- ``planted_decoder.box_rays``:
origins 1.5 from the object's centre, three quarters of them aimed into the box, depths 0.75 .. 2.25 -- are mapped through the inverse
geometry to the sampling frame,

    o = M^-1 o' xyz_div[b] / xyz_mul,   d = M^-1 d' / |M^-1 d'|,   t = t' |M^-1 d'| xyz_div[b] / xyz_mul      (per-ray depths)

so that the decoder sees o' + t' d' again.  Depth tables that several rays share cannot carry the per-ray factor |M^-1 d'| (0.9 .. 1.1 with
the frames below): a per-object row is t'_b xyz_div[b] / xyz_mul, and the shared row is t' DIV_MID / xyz_mul with every object's decoder-frame
rays scaled by DIV_MID / xyz_div[b] (0.8 .. 1.25: the same metric scene seen by objects of different size), which keeps the decoder-frame
points within 1.25 x 1.1 of where ``box_rays`` has them (at most 1.5 from the centre: the far end of a ray that misses).  SNR_Z_BOX: o = M^-1 o' z_scale[b] / xyz_mul, and the depths are the kernel's own, between the bounds of box b."""
import math
from typing import NamedTuple, Optional

import torch

import planted_decoder as PD
from oracle import supnerf_oracle as O

XYZ_MUL = 0.9                    # the fixture's adjust_scale (tests/golden/render_v3_b_hit.npz)
# neither orthogonal (|M M^T - 1| = 0.12) nor symmetric (|M - M^T| = 0.38); singular values 0.93 .. 1.10, condition number 1.19
FRAME_GENERAL = (0.93, 0.21, -0.12,
                 -0.17, 1.04, 0.09,
                 0.08, -0.19, 0.97)
MAX_OBJECTS = 7


def frame_flags():
    """``utils._frame(True, True, True)``: the reference's three edits composed (y mirror, KITTI -> nuScenes, nuScenes -> ShapeNet), a signed
    permutation that is not symmetric."""
    from supnerf_amd import utils
    return utils._frame(True, True, True)


def frame_of(name):
    return FRAME_GENERAL if name == "general" else frame_flags()


def xyz_div(B):
    """(B,) float64, like obj_diag of family A: distinct, no power of two."""
    return torch.tensor([1.13 + 0.17 * b for b in range(B)], dtype=torch.float64)


def z_scale(B):
    """(B,) float64, like obj_diag / 2 of family B: distinct, no power of two, falling where xyz_div rises."""
    return torch.tensor([2.6 - 0.23 * b for b in range(B)], dtype=torch.float64)


def box_half(B):
    """(B,3) float64: the planted box's outer surface, +-(HALF + H), stretched differently per object and axis."""
    h = torch.tensor([v + PD.H for v in PD.HALF], dtype=torch.float64)
    b = torch.arange(1, B + 1, dtype=torch.float64)[:, None]
    return h[None] + b * torch.tensor([0.03, -0.02, 0.025], dtype=torch.float64)[None]


# (z mode, samples per ray, rays per object, objects): each the smallest shape that reaches its seam
RAW_CASES = [
    ("per_ray", 4, 3, 7),        # 12 points per object: five objects inside a 64-point workgroup, rem0 != 0 in the second, a partial last one
    ("shared", 8, 5, 4),
    ("per_object", 16, 3, 3),
    ("box", 4, 24, 3),           # 96 points per object: rem0 = 16 with an object boundary inside the workgroup
    ("per_ray", 64, 1, 3),       # one ray = one object = one workgroup
    ("per_ray", 128, 1, 3),      # the WAVES = 8 forward and the 32x32x2 backward: rays_per_obj < wgp, one ray per workgroup
    ("box", 128, 1, 3),
]
MODULE_CASES = [
    ("per_ray", 8, 1, 3),        # one ray per object, padded to 4 rays: a (B,) z_scale has as many entries as there are rays
    ("box", 8, 1, 3),
    ("per_object", 32, 3, 5),    # 96 points per object: the fp32 backward falls to the 32x32 kernel, objects straddle forward workgroups
    ("box", 16, 6, 4),
    ("per_ray", 64, 2, 3),       # the two-waves backward with latent rows
    ("shared", 32, 2, 3),
    ("per_ray", 4, 8, 5),        # two objects per 64-point workgroup
]
BOTH_FRAMES = {("raw", ("per_ray", 4, 3, 7)), ("module", ("per_object", 32, 3, 5)), ("module", ("box", 16, 6, 4))}
# (route, case, frame name)
RUNS = [(route, c, f) for route, cases in (("raw", RAW_CASES), ("module", MODULE_CASES)) for c in cases
        for f in (("general", "flags") if (route, c) in BOTH_FRAMES else ("general",))]
RUN_ID = lambda r: f"{r[0]}-{r[1][0]}-S{r[1][1]}-n{r[1][2]}-B{r[1][3]}-{r[2]}"


class Launch(NamedTuple):
    """The operands of one launch, fp32 as the kernels take them (``frame`` and ``xyz_mul`` rounded to fp32 like the C struct's fields)."""
    mode: str
    S: int
    n: int
    B: int
    rays_o: torch.Tensor          # (N,3) sampling frame
    rays_d: torch.Tensor          # (N,3) unit
    t_vals: torch.Tensor          # depths in the mode's layout; "box": the (N,S) jitter
    xyz_div: torch.Tensor         # (B,)
    z_scale: torch.Tensor         # (B,)
    box_half: Optional[torch.Tensor]   # (B,3), "box" only
    frame: torch.Tensor           # (3,3) fp32
    xyz_mul: float
    codes: tuple                  # shape / texture codes (B,256), distinct per object
    latent: torch.Tensor          # (B,4,256) latent terms for the raw operators, distinct per object
    wts: tuple                    # upstream weights of rgb (N,3), depth (N), acc (N): random per ray


def seed_of(case, frame_name):
    _, S, n, B = case
    return 7 * S + 3 * n + 11 * B + (1000 if frame_name != "general" else 0)


def planned_rays(case, frame_name="general"):
    """The decoder-frame rays a case is built from: ``box_rays`` o', d' (N,3) and t' (N,S), float64."""
    _, S, n, B = case
    return PD.box_rays(B * n, S, seed=seed_of(case, frame_name), dtype=torch.float64)


def build(case, frame_name="general") -> Launch:
    mode, S, n, B = case
    assert B <= MAX_OBJECTS
    N = B * n
    seed = seed_of(case, frame_name)
    g = torch.Generator().manual_seed(seed)
    f32 = lambda x: x.to(torch.float32)
    M = f32(torch.tensor(frame_of(frame_name), dtype=torch.float64).reshape(3, 3)).double()
    mul = float(f32(torch.tensor(XYZ_MUL)))
    Minv = torch.linalg.inv(M)
    div, zs, half = xyz_div(B), z_scale(B), box_half(B)
    obj = torch.arange(N) // n
    o1, d1, t1 = planned_rays(case, frame_name)
    dm = d1 @ Minv.T
    stretch = dm.norm(dim=-1, keepdim=True)
    d = dm / stretch
    if mode == "box":
        o = (o1 @ Minv.T) * (zs[obj][:, None] / mul)
        t = torch.rand(N, S, generator=g, dtype=torch.float64)
    else:
        div_mid = math.sqrt(float(div[0] * div[-1]))
        s = (div_mid / div[obj])[:, None] if mode == "shared" else torch.ones(N, 1, dtype=torch.float64)
        o = (o1 * s) @ Minv.T * (div[obj][:, None] / mul)
        grid = torch.linspace(0.75, 2.25, S + 1, dtype=torch.float64)[:-1]
        if mode == "per_ray":
            t = t1 * stretch * (div[obj][:, None] / mul)
        elif mode == "per_object":
            t = (grid[None] + torch.rand(B, S, generator=g, dtype=torch.float64) * (1.5 / S)) * (div[:, None] / mul)
        else:
            t = (grid + torch.rand(S, generator=g, dtype=torch.float64) * (1.5 / S)) * (div_mid / mul)
    sc, tc = [torch.randn(B, 256, generator=g) * 0.3 for _ in range(2)]
    lat = torch.relu(torch.randn(B, 4, 256, generator=g) * 0.3)
    wts = (torch.randn(N, 3, generator=g), torch.randn(N, generator=g), torch.randn(N, generator=g))
    return Launch(mode, S, n, B, f32(o), f32(d), f32(t), f32(div), f32(zs), f32(half) if mode == "box" else None, f32(M), mul, (sc, tc),
                  lat, wts)


def decoder_frame_points(c: Launch):
    """Where the decoder sees the launch's samples, float64: p (N,S,3), and the hit mask ("box") or None."""
    with torch.no_grad():
        obj = torch.arange(c.B * c.n) // c.n
        o, d, zs = c.rays_o.double(), c.rays_d.double(), c.z_scale.double()[obj]
        hit = None
        if c.mode == "box":
            o = o / zs[:, None]
            h = c.box_half.double()[obj]
            near, far, hit = O.slab_intersect(o, d, -h, h)
            minus1 = torch.full_like(near, -1.0)
            t = O.unit_interval_samples(torch.where(hit, near, minus1)[:, None], torch.where(hit, far, minus1)[:, None], c.S, c.t_vals.double())
            scale = torch.ones_like(zs)
        else:
            t = {"shared": lambda: c.t_vals[None].expand(c.B * c.n, c.S), "per_object": lambda: c.t_vals[obj], "per_ray": lambda: c.t_vals}[c.mode]().double()
            scale = 1.0 / c.xyz_div.double()[obj]
        p = (o[:, None, :] + t[:, :, None] * d[:, None, :]) * (scale[:, None, None] * c.xyz_mul)
        return p @ c.frame.double().T, hit


# the wrong geometries a test must be able to see (test_render_geometry_cpu.py): name -> what it changes
WRONG = ("xyz_div_rolled", "z_scale_rolled", "box_half_rolled", "frame_transposed", "xyz_mul_one", "obj_of_previous")


def oracle(params, c: Launch, dt, masks=None, latent=None, lat_on=None, wrong=None):
    """The launch on the oracle in dtype ``dt`` (white background, metric depths), and the gradients of sum(outputs * wts): dict of rgb,
    depth, acc, d_rays_o, d_rays_d, d_t (per-ray depths), d_latent, d_shapecode, d_texturecode.  The latent terms are ``latent`` as given
    (the raw operators), else those of the launch's codes with the ReLU derivative ``lat_on``.  ``wrong``: one of ``WRONG``."""
    p = {k: v.to(dt) for k, v in params.items()}
    N = c.B * c.n
    ro, rd = c.rays_o.to(dt).clone().requires_grad_(), c.rays_d.to(dt).clone().requires_grad_()
    t = c.t_vals.to(dt).clone().requires_grad_() if c.mode == "per_ray" else c.t_vals.to(dt)
    sc = tc = None
    if latent is not None:
        lat = latent.to(dt).clone().requires_grad_()
    else:
        sc, tc = [x.to(dt).clone().requires_grad_() for x in c.codes]
        lat = O.latent_terms(p, sc, tc, relu_mask=lat_on)
        lat.retain_grad()
    div, zs, half, frame, mul, obj = c.xyz_div.to(dt), c.z_scale.to(dt), None if c.box_half is None else c.box_half.to(dt), c.frame.to(dt), c.xyz_mul, None
    if wrong == "xyz_div_rolled":
        div = div.roll(1)
    elif wrong == "z_scale_rolled":
        zs = zs.roll(1)
    elif wrong == "box_half_rolled":
        half = half.roll(1, 0)
    elif wrong == "frame_transposed":
        frame = frame.T.contiguous()
    elif wrong == "xyz_mul_one":
        mul = 1.0
    elif wrong == "obj_of_previous":          # the first ray behind every object boundary takes the previous object's constants
        obj = torch.arange(N) // c.n
        first = torch.arange(1, c.B) * c.n
        obj[first] -= 1
    else:
        assert wrong is None, wrong
    out = O.fused_render(p, ro, rd, t, c.mode, c.S, c.n, zs, half, latent=lat, relu_masks=masks, white_bkgd=True, metric_z=True,
                         xyz_div=div, xyz_mul=mul, frame=frame, obj=obj)
    sum((a * w.to(dt)).sum() for a, w in zip(out, c.wts)).backward()
    g = lambda x: None if x is None else x.grad
    return dict(rgb=out[0].detach(), depth=out[1].detach(), acc=out[2].detach(), d_rays_o=ro.grad, d_rays_d=rd.grad,
                d_t=t.grad if c.mode == "per_ray" else None, d_latent=lat.grad, d_shapecode=g(sc), d_texturecode=g(tc))
