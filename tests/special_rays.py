"""Test helper: rays on which the box sampler (``SNR_Z_BOX``) has to follow a rule instead of a formula, and how to plant them in a batch.

The rays are given in the box frame of the table's box, half extents ``HB`` = (.5, .25, .125), and are built from dyadic numbers, so every
product and difference of the slab test is exact in float32 and in float64 and every tie is a tie in both.  Directions are not unit
vectors: nothing in the prologue normalises them.  The classes (``Ray.cls``):

* ``parallel``     two direction components exactly 0 (one of them -0.0 once), origin strictly inside both slabs: a hit;
* ``zero_in``      one component 0 (+0.0 or -0.0), origin strictly inside that slab: a hit, and that axis adds nothing to any gradient;
* ``zero_out``     component(s) 0 with the origin outside that slab: a miss (t_far = -inf or t_near = +inf);
* ``zero_face``    component 0 with the origin ON that face: 0 * inf = NaN in the slab test -> a miss, and the NaN reaches no output;
* ``tie``          entry or exit through an edge / a corner: the bound's gradient splits 1/2-1/2 / 1/4-1/4-1/2 (two nested maximum);
* ``inside``       origin inside the box: a hit with near < 0 < far;
* ``face_in``      origin on a face, pointing in: near = 0 exactly; with jitter 0 at sample 0 the first point is the origin, depth 0;
* ``behind``       the box lies behind the origin: a miss (t_far < 0);
* ``graze``        the ray touches an edge only, t_near == t_far: a miss (the comparison is strict).

``embed`` plants them among generic rays (``planted_decoder.box_rays``) in a batch of B objects x n rays, each object with its own box (the
table's scaled by a power of two, origins scaled with it) and its own power-of-two ``z_scale``."""
import math
from collections import namedtuple

import torch

import planted_decoder as PD
from oracle import supnerf_oracle as O

INF = float("inf")
HB = (0.5, 0.25, 0.125)
P7 = 2.0 ** -7

# near / far: the exact bounds of a hit (None: not listed); zero_axes: the axes with d == 0 and the origin strictly inside their slab (hits)
Ray = namedtuple("Ray", "name cls o d hit near far zero_axes")

TABLE = [
    Ray("par +z", "parallel", (.125, .0625, -2), (0., 0., 1.), True, 1.875, 2.125, (0, 1)),
    Ray("par -z", "parallel", (.125, .0625, 2), (0., 0., -1.), True, 1.875, 2.125, (0, 1)),
    Ray("par +x (-0, 0)", "parallel", (-3, .0625, .03125), (1., -0., 0.), True, 2.5, 3.5, (1, 2)),
    Ray("par +y", "parallel", (.125, -2, .03125), (0., 1., 0.), True, 1.75, 2.25, (0, 2)),
    Ray("par -y (-0, -0)", "parallel", (-.25, 2, -.0625), (-0., -1., -0.), True, 1.75, 2.25, (0, 2)),
    Ray("dx=0", "zero_in", (.125, -1, -1.5), (0., .6, .8), True, None, None, (0,)),
    Ray("dy=-0", "zero_in", (-2, .0625, -1.5), (.8, -0., .6), True, None, None, (1,)),
    Ray("dz=0", "zero_in", (-2, -1, .03125), (.8, .6, 0.), True, None, None, (2,)),
    Ray("dx=0 outside slab", "zero_out", (.75, -1, -1.5), (0., .6, .8), False, None, None, ()),
    Ray("par +z outside two slabs", "zero_out", (.75, -.5, -2), (0., -0., 1.), False, None, None, ()),
    Ray("dx=0 on face", "zero_face", (.5, -1, -1.5), (0., .6, .8), False, None, None, ()),
    Ray("dx=-0 on face -hb", "zero_face", (-.5, -1, -1.5), (-0., .6, .8), False, None, None, ()),
    Ray("par +z on face y", "zero_face", (.125, .25, -2), (0., 0., 1.), False, None, None, ()),
    Ray("edge entry tie", "tie", (-1.5, .0625, -1.125), (.5, P7, .5), True, 2., 2.5, ()),
    Ray("corner entry tie", "tie", (-1.5, -1.25, -1.125), (.5, .5, .5), True, 2., 2.5, ()),
    Ray("edge entry tie, d_z < 0", "tie", (-1.5, .0625, 1.125), (.5, P7, -.5), True, 2., 2.5, ()),
    Ray("edge exit tie", "tie", (-1., .0625, -1.375), (.5, P7, .5), True, 2.5, 3., ()),
    Ray("corner exit tie", "tie", (-1., -1.25, -1.375), (.5, .5, .5), True, 2.5, 3., ()),
    Ray("inside", "inside", (.125, .0625, .03125), (.6, .48, .64), True, None, None, ()),
    Ray("centre", "inside", (0., 0., 0.), (.6, .48, .64), True, None, None, ()),
    Ray("on face x pointing in", "face_in", (-.5, .0625, .03125), (1., .125, .0625), True, 0., 1., ()),
    Ray("on face z pointing in", "face_in", (.125, .0625, .125), (.25, .125, -1.), True, 0., .25, ()),
    Ray("box behind", "behind", (.125, .0625, 2), (.28, 0., .96), False, None, None, ()),
    Ray("box behind, generic direction", "behind", (.125, .0625, 2), (.25, .125, 1.), False, None, None, ()),
    Ray("touches an edge", "graze", (-1.5, .0625, -.875), (.5, P7, .5), False, None, None, ()),
    Ray("touches a corner", "graze", (-1.5, -1.25, -.875), (.5, .5, .5), False, None, None, ()),
]
CLASSES = ("parallel", "zero_in", "zero_out", "zero_face", "tie", "inside", "face_in", "behind", "graze")
# the pairs of axes whose entry (lo) or exit (hi) depths tie exactly, and the share of the bound's gradient each axis takes
TIES = {"edge entry tie": ("lo", {0: .5, 1: 0., 2: .5}), "corner entry tie": ("lo", {0: .25, 1: .25, 2: .5}),
        "edge entry tie, d_z < 0": ("lo", {0: .5, 1: 0., 2: .5}), "edge exit tie": ("hi", {0: .5, 1: 0., 2: .5}),
        "corner exit tie": ("hi", {0: .25, 1: .25, 2: .5})}


def table_tensors(dtype=torch.float32):
    """(origins (T,3), directions (T,3), half extents (T,3)) of the table in ``dtype``."""
    o = torch.tensor([r.o for r in TABLE], dtype=dtype)
    d = torch.tensor([r.d for r in TABLE], dtype=dtype)
    return o, d, torch.tensor(HB, dtype=dtype).expand_as(o).contiguous()


def slab_axes(o, d, hb):
    """Per axis entry / exit depths (lo, hi) of the plain slab test: the quantities that tie."""
    inv = torch.reciprocal(d)
    ta, tb = (-hb - o) * inv, (hb - o) * inv
    return torch.minimum(ta, tb), torch.maximum(ta, tb)


def bounds_of(slab, o, d, hb):
    """(near, far, hit) of a slab function after the reference's -1 / -1 substitution on misses."""
    tn, tf, hit = slab(o, d, -hb, hb)
    m1 = torch.full_like(tn, -1.0)
    return torch.where(hit, tn, m1), torch.where(hit, tf, m1), hit


# ------------------------------------------------------------------ deliberately wrong references (tests/test_special_rays_cpu.py)
def _pick_first(a, b, larger):
    """max / min whose whole gradient goes to the first argument on a tie (share 1 / 0 where torch splits 1/2 - 1/2)."""
    pick = torch.where(a >= b, a, b) if larger else torch.where(a <= b, a, b)
    return torch.where(torch.isnan(a) | torch.isnan(b), a + b, pick)             # (a NaN stays the result, as in torch.maximum)


def tie_mutant_slab(o, d, bmin, bmax):
    """``O.guarded_slab_intersect`` with 1 / 0 tie shares across the axes: the same values, a wrong gradient on tie rays only."""
    lo, hi = O.guarded_slab_axes(o, d, bmin, bmax)
    t_near = _pick_first(_pick_first(lo[..., 0], lo[..., 1], True), lo[..., 2], True)
    t_far = _pick_first(_pick_first(hi[..., 0], hi[..., 1], False), hi[..., 2], False)
    hit = t_far > t_near
    return t_near, t_far, hit & ((t_far * hit) > 0)


def whole_ray_drop_slab(o, d, bmin, bmax):
    """The cheap wrong fix of the 0 * inf gradient: the bounds' path dropped on the WHOLE ray that has a zero direction component, where
    only that component's axis contributes nothing."""
    t_near, t_far, hit = O.guarded_slab_intersect(o, d, bmin, bmax)
    any_zero = (d == 0).any(-1)
    return torch.where(any_zero, t_near.detach(), t_near), torch.where(any_zero, t_far.detach(), t_far), hit


# ------------------------------------------------------------------ the table inside a batch
OBJ_SCALE = (1.0, 0.5, 0.25)          # object b's box is the table's times OBJ_SCALE[b % 3]; its special origins scale with it
OBJ_Z_SCALE = (2.0, 4.0, 1.0)         # rays_o = box-frame origin * z_scale: exact, and the kernel's rays_o / z_scale gives it back


def launch_rays(n, S):
    """Rays per object of the launch: the operators pad every object to whole 32-point wave tiles when the codes need a gradient."""
    if (n * S) % 32 == 0:
        return n
    step = 32 // math.gcd(32, S)
    return -(-n // step) * step


Batch = namedtuple("Batch", "rays_o rays_d half z_scale jitter special n B S")
Special = namedtuple("Special", "index obj local ray scale")         # index into the batch, object, ray within it, TABLE entry, box scale


def embed(n, B, S, seed=0):
    """A batch of B objects x n rays with the table planted in it: every object holds the whole table when n allows it, else the table is
    dealt to the objects in turn (B * n >= len(TABLE) is required).  Within an object the special rays take, first, the places that are
    the first / last ray of the object, of a 128-point workgroup tile and of a 64-point tile of the (padded) launch, then places drawn by
    a fixed permutation; every other place holds a generic ray.  The jitter (N,S) is random with exact zeros in it: sample 0 of every
    special ray, and one in sixteen entries elsewhere."""
    T = len(TABLE)
    assert B * n >= T, (B, n, T)
    g = torch.Generator().manual_seed(1000 * seed + 31 * n + 7 * B + S)
    go, gd, _ = PD.box_rays(B * n, S, seed=seed + n + B)
    scale = torch.tensor([OBJ_SCALE[b % 3] for b in range(B)])
    zs = torch.tensor([OBJ_Z_SCALE[b % 3] for b in range(B)])
    o_n = go.view(B, n, 3) * 2.0 * scale[:, None, None]             # (generic rays: from radius 3 s at a box of half extents HB s)
    d = gd.view(B, n, 3).clone()
    jitter = torch.rand(B * n, S, generator=g)
    jitter[torch.rand(B * n, S, generator=g) < 1 / 16] = 0.0
    jitter = jitter.view(B, n, S)
    deal = [list(range(T)) for _ in range(B)] if n >= T else [list(range(b, T, B)) for b in range(B)]
    n_l, r128, r64 = launch_rays(n, S), max(128 // S, 1), max(64 // S, 1)
    special, covered = [], set()
    for b in range(B):
        pos = lambda r: b * n_l + r                                  # the ray's index in the launch
        want = {"obj_first": [0], "obj_last": [n - 1],
                "t128_first": [r for r in range(n) if pos(r) % r128 == 0], "t128_last": [r for r in range(n) if pos(r) % r128 == r128 - 1],
                "t64_first": [r for r in range(n) if pos(r) % r64 == 0], "t64_last": [r for r in range(n) if pos(r) % r64 == r64 - 1]}
        places = []
        for key, cand in want.items():
            if cand and len(places) < len(deal[b]) and not (set(cand) & set(places)):
                places.append(cand[0] if key.endswith("first") else cand[-1])
        rest = [r for r in torch.randperm(n, generator=g).tolist() if r not in places]
        places += rest[:len(deal[b]) - len(places)]
        for key, cand in want.items():
            if set(cand) & set(places):
                covered.add(key)
        order = torch.randperm(len(deal[b]), generator=g).tolist()  # which special ray takes which place changes with the case
        for k, r in zip(order, places):
            ray = TABLE[deal[b][k]]
            o_n[b, r] = torch.tensor(ray.o) * scale[b]
            d[b, r] = torch.tensor(ray.d)
            jitter[b, r, 0] = 0.0
            special.append(Special(b * n + r, b, r, ray, float(scale[b])))
    assert len(covered) == 6, f"no special ray at {sorted(set(['obj_first', 'obj_last', 't128_first', 't128_last', 't64_first', 't64_last']) - covered)}"
    assert sorted(set(s.ray.name for s in special)) == sorted(r.name for r in TABLE)
    half = torch.tensor(HB)[None, :] * scale[:, None]
    rays_o = (o_n * zs[:, None, None]).reshape(B * n, 3).contiguous()
    special.sort(key=lambda s: s.index)
    return Batch(rays_o, d.reshape(B * n, 3).contiguous(), half.contiguous(), zs, jitter.reshape(B * n, S).contiguous(), special, n, B, S)


def rays_of(batch, pred):
    """Indices (into the batch) and names of the special rays for which ``pred(Special)`` holds."""
    sel = [s for s in batch.special if pred(s)]
    return [s.index for s in sel], [f"{s.ray.name} [obj {s.obj} ray {s.local}]" for s in sel]


def count_by_class(batch, idx):
    """{class: how many of the batch rays ``idx`` are special rays of it}, every class present (0 where none)."""
    by = {s.index: s.ray.cls for s in batch.special}
    out = {c: 0 for c in CLASSES}
    for i in idx:
        out[by[int(i)]] += 1
    return out


# ------------------------------------------------------------------ one render case: inputs and the oracle's side of it
Case = namedtuple("Case", "batch codes wts")


def case_inputs(n, B, S):
    """The batch, the objects' codes (B,256) x 2 and the upstream weights of (rgb, depth, acc) of one (rays per object, objects, samples)
    case: what tests/test_special_rays_gpu.py launches and tests/test_special_rays_cpu.py shows the bands to be sensitive on."""
    batch = embed(n, B, S)
    g = torch.Generator().manual_seed(77 + S + 3 * n + 11 * B)
    codes = [torch.randn(B, 256, generator=g) * 0.3 for _ in range(2)]
    N = B * n
    s = (2.0 ** torch.arange(B)).repeat_interleave(n)              # distinct upstream scales per object
    wts = [torch.randn(N, 3, generator=g) * s[:, None], torch.randn(N, generator=g) * s, torch.randn(N, generator=g) * s]
    # On a special ray the depth weighs 3 .. 4 (either sign) and the transmittance 24 .. 32 with the opposite sign.  In the suite's decoder, a thin fog, the depth
    # moves with the far bound (the last, 1e10-wide sample takes most of the weight) and the transmittance with far - near, so these two
    # add up in the far bound, do not cancel in the near one, and make both bounds' paths a fair share of the ray's gradient whatever the other draws are -- the condition test_special_rays_cpu.py
    # checks: a wrong path through either bound shows in the per-ray band.
    idx = torch.tensor([sp.index for sp in batch.special])
    sign = lambda w: torch.where(w < 0, -1.0, 1.0)
    wts[1][idx] = sign(wts[1][idx]) * (3 + torch.rand(len(idx), generator=g)) * s[idx]
    wts[2][idx] = -sign(wts[1][idx]) * (24 + 8 * torch.rand(len(idx), generator=g)) * s[idx]
    return Case(batch, codes, wts)


def oracle_render(params, case, dt, slab=None, masks=None, lat_on=None, box_detach=False):
    """The fused box render of ``case`` on the oracle in dtype ``dt`` (white background, metric depth) with the slab test ``slab``
    (default: the guarded one) and its gradients: dict of rgb, depth, acc, d_rays_o, d_rays_d, d_latent, d_shapecode, d_texturecode."""
    b = case.batch
    p = {k: v.to(dt) for k, v in params.items()}
    ro, rd = b.rays_o.to(dt).clone().requires_grad_(), b.rays_d.to(dt).clone().requires_grad_()
    sc, tc = [c.to(dt).clone().requires_grad_() for c in case.codes]
    lat = O.latent_terms(p, sc, tc, relu_mask=lat_on)
    lat.retain_grad()
    out = O.fused_render(p, ro, rd, b.jitter.to(dt), "box", b.S, b.n, b.z_scale.to(dt), b.half.to(dt), latent=lat, relu_masks=masks,
                         white_bkgd=True, metric_z=True, slab=slab or O.guarded_slab_intersect, box_detach=box_detach)
    sum((a * w.to(dt)).sum() for a, w in zip(out, case.wts)).backward()
    return dict(rgb=out[0].detach(), depth=out[1].detach(), acc=out[2].detach(), d_rays_o=ro.grad, d_rays_d=rd.grad, d_latent=lat.grad,
                d_shapecode=sc.grad, d_texturecode=tc.grad)


# (S, rays per object, objects) and, per arithmetic of the backward, the kernel and tail it reaches (tests/test_special_rays_gpu.py's
# docstring).  Rays per object >= len(TABLE) wherever the whole table fits an object.
CASES = [
    (4, 32, 1), (4, 32, 3), (8, 32, 3), (16, 28, 1),        # points per object % 64 == 0, S <= 16: fp32 two-wave, in-wave finish
    (32, 26, 3), (64, 26, 1), (64, 26, 3),                  # ... S = 32, 64: fp32 two-wave, LDS combine
    (4, 40, 3), (8, 28, 1), (16, 26, 3), (32, 27, 3),       # points per object % 64 == 32: fp32 round-2, in-wave finish
    (128, 26, 3), (128, 9, 3),                              # S = 128: fp32 round-2, LDS combine (the second: the table dealt over 3 objects)
    (8, 27, 3), (16, 27, 1),                                # ragged: 216 / 432 points per object, padded to 28 rays: fp32 round-2 / two-wave
]
