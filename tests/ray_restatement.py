"""Test helper: the ray-surface rules of include/supnerf_hip.h ("Ray-cast surfaces") restated in numpy, one written operation per
rounding, for any density callable -- what ``snr_ray_march_points``, ``snr_ray_first_crossing`` and ``snr_ray_hit_points`` compute bit for
bit when the callable returns the GPU's own sigma -- plus the float64 side the tests judge it by: a dense float64 march with bisection (the
true first crossing), the oracle decoder's density chain on its own, and rule 8 (the implicit-function gradient) in any dtype.

A density callable takes points (P, 3) float32, ray-major (object-major over the objects of a launch), and returns sigma (P,) float32."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import supnerf_oracle as O

f32 = np.float32


# ------------------------------------------------------------------ rules 1 - 6, float32
def march_t(ta, tb, S):
    """Rule 1: (R, S) depths of the march of [ta, tb]: ta + step k with step = (tb - ta) / (S - 1); the last column is tb itself."""
    ta, tb = np.asarray(ta, f32), np.asarray(tb, f32)
    step = ((tb - ta) / f32(S - 1)).astype(f32)
    t = (ta[:, None] + (step[:, None] * np.arange(S, dtype=f32)[None, :]).astype(f32)).astype(f32)
    t[:, S - 1] = tb
    return t


def march_points(o, d, ta, tb, S):
    """Rule 1: the (R S, 3) point list, p = o + t d per axis (one multiply, one add)."""
    o, d = np.asarray(o, f32), np.asarray(d, f32)
    t = march_t(ta, tb, S)
    return (o[:, None, :] + (t[:, :, None] * d[:, None, :]).astype(f32)).astype(f32).reshape(-1, 3)


def inside(sig, level):
    """Rule 2: sigma >= level; a NaN is outside."""
    with np.errstate(invalid="ignore"):
        return np.asarray(sig, f32) >= f32(level)


def first_crossing(sig, ta, tb, level, bracket=None):
    """Rules 3 - 5 on sigma (R, S), the densities of the march of [ta, tb].  ``bracket`` None: the first march -> (ta', tb', va, vb,
    state); a ray of state 0 / 2 leaves with [ta, ta], va = vb = 0.  ``bracket`` = (va, vb, state) of the march before: a refinement;
    only state-1 rays are searched, and one without a crossing keeps what it had.  Returns new arrays, and the state-1 rays that found
    no crossing as a sixth value (rule 5 says there are none when sigma is the decoder's)."""
    sig = np.asarray(sig, f32)
    R, S = sig.shape
    ta, tb = np.asarray(ta, f32).copy(), np.asarray(tb, f32).copy()
    ins = inside(sig, level)
    cross = ~ins[:, :-1] & ins[:, 1:]
    has = cross.any(axis=1)
    k = np.where(has, cross.argmax(axis=1), 0)
    t = march_t(ta, tb, S)
    rows = np.arange(R)
    if bracket is None:
        state = np.where(ins[:, 0], 2, np.where(has, 1, 0)).astype(np.uint8)
        take = state == 1
        va, vb = np.zeros(R, f32), np.zeros(R, f32)
        lost = np.zeros(R, bool)
        tb[~take] = ta[~take]
    else:
        va, vb, state = [np.asarray(x).copy() for x in bracket]
        take = (state == 1) & has
        lost = (state == 1) & ~has
    ta[take], tb[take] = t[rows, k][take], t[rows, k + 1][take]
    va[take], vb[take] = sig[rows, k][take], sig[rows, k + 1][take]
    return ta, tb, va, vb, state, lost


def hit_points(o, d, ta, tb, va, vb, state, level):
    """Rule 6: (depth, width, x): t = ta + (level - va) / (vb - va) * (tb - ta) and width tb - ta on state 1; t = ta on state 2; 0 on
    state 0; x = o + t d for every ray."""
    o, d = np.asarray(o, f32), np.asarray(d, f32)
    hit = state == 1
    with np.errstate(all="ignore"):
        w = (tb - ta).astype(f32)
        q = ((f32(level) - va).astype(f32) / (vb - va).astype(f32)).astype(f32)
        t1 = (ta + (q * w).astype(f32)).astype(f32)
    t = np.where(hit, t1, np.where(state == 2, ta, f32(0))).astype(f32)
    width = np.where(hit, w, f32(0)).astype(f32)
    x = (o + (t[:, None] * d).astype(f32)).astype(f32)
    return t, width, x


def ray_surface(sigma_fn, o, d, near, far, level, n_samples, refine=(0, 2)):
    """Rules 1 - 6 from end to end.  Returns a dict: depth, width, x, state, the final bracket (ta, tb, va, vb), per march the point list,
    sigma and bracket (``marches``), and ``lost``: how many state-1 rays had no crossing in some refinement march."""
    o, d = np.asarray(o, f32), np.asarray(d, f32)
    R = o.shape[0]
    ta, tb = np.broadcast_to(np.asarray(near, f32), (R,)).copy(), np.broadcast_to(np.asarray(far, f32), (R,)).copy()
    levels, s_r = refine
    bracket, marches, lost = None, [], 0
    for S in [n_samples] + [s_r] * levels:
        pts = march_points(o, d, ta, tb, S)
        sig = np.asarray(sigma_fn(pts), f32).reshape(R, S)
        ta, tb, va, vb, state, gone = first_crossing(sig, ta, tb, level, bracket)
        bracket = (va, vb, state)
        lost += int(gone.sum())
        marches.append(dict(points=pts, sigma=sig, ta=ta.copy(), tb=tb.copy(), va=va.copy(), vb=vb.copy()))
    t, width, x = hit_points(o, d, ta, tb, va, vb, state, level)
    return dict(depth=t, width=width, x=x, state=state, ta=ta, tb=tb, va=va, vb=vb, marches=marches, lost=lost)


# ------------------------------------------------------------------ rules 7 - 8, any dtype (torch)
def normals(g, state):
    """Rule 7: -g / |g| on state 1 where |g| is finite and not zero, else the zero vector."""
    g = torch.as_tensor(g)
    norm = g.norm(dim=1, keepdim=True)
    good = torch.as_tensor(np.asarray(state) == 1)[:, None] & torch.isfinite(norm) & (norm > 0)
    return torch.where(good, -g / torch.where(good, norm, torch.ones_like(norm)), torch.zeros_like(g))


def implicit_gradient(g, d, t, state, d_t):
    """Rule 8: with slope = g . d (summed in axis order) and c = -d_t / slope on state 1, 0 elsewhere: (d o = c g, d d = t c g, c);
    c is the d sigma the density backward takes for the gradient to the codes."""
    g, d, t, d_t = [torch.as_tensor(x) for x in (g, d, t, d_t)]
    slope = g[:, 0] * d[:, 0] + g[:, 1] * d[:, 1] + g[:, 2] * d[:, 2]
    hit = torch.as_tensor(np.asarray(state) == 1)
    c = torch.where(hit, -d_t / slope, torch.zeros_like(t))
    return c[:, None] * g, (t * c)[:, None] * g, c


# ------------------------------------------------------------------ the oracle decoder's density, and the float64 truth
def oracle_sigma(params, xyz, shape_code, relu_masks=None):
    """sigma (P,) of the oracle decoder at points (P, 3), object-major over the codes (B, 256): ``O.decoder_forward``'s chain up to the
    density head and nothing after it (the same operations in the same order: the same bits), in the dtype of ``params``.
    ``relu_masks``: 0/1 tensors for encoding_xyz and the shape layers whose entries replace the ReLUs' derivatives, as in the oracle."""
    sb, _ = O._count_blocks(params)
    x = xyz.view(-1, 1, 3)
    rows = shape_code.repeat_interleave(x.shape[0] // shape_code.shape[0], dim=0).unsqueeze(1)
    lin = lambda name, t: F.linear(t, params[name + ".weight"], params[name + ".bias"])
    i = [0]

    def relu(t):
        if relu_masks is None:
            return F.relu(t)
        i[0] += 1
        return O._ReluWithGivenMask.apply(t, relu_masks[i[0] - 1].reshape(t.shape))
    h = relu(lin("encoding_xyz.0", O.positional_encoding(x, 10)))
    for j in range(1, sb + 1):
        h = relu(lin(f"shape_layer_{j}.0", h + F.relu(lin(f"shape_latent_layer_{j}.0", rows))))
    return F.softplus(lin("sigma.0", lin("encoding_shape", h))).view(-1)


def oracle_sigma_fn(params, shape_code, chunk=1 << 16):
    """``oracle_sigma`` as a density callable in the dtype of ``params`` (numpy in, numpy out, evaluated in chunks per object)."""
    dt = params["sigma.0.weight"].dtype
    B = shape_code.shape[0]

    def fn(pts):
        p = torch.as_tensor(np.asarray(pts)).to(dt).view(B, -1, 3)
        out = []
        with torch.no_grad():
            for b in range(B):
                out.append(torch.cat([oracle_sigma(params, p[b, i:i + chunk], shape_code[b:b + 1].to(dt)) for i in range(0, p.shape[1], chunk)])
                           if p.shape[1] else p.new_zeros(0))
        return torch.cat(out).numpy()
    return fn


def truth(sigma64, o, d, near, far, level, n_march=4001, n_bisect=40):
    """The first crossing in float64: a march of ``n_march`` samples with ``sigma64`` (points (P, 3) float64 numpy -> sigma float64), then
    ``n_bisect`` bisections of its first outside -> inside pair.  Returns (state, depth): depth the bracket's midpoint on state 1,
    near on state 2, 0 on state 0."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    R = o.shape[0]
    near, far = np.broadcast_to(np.asarray(near, np.float64), (R,)), np.broadcast_to(np.asarray(far, np.float64), (R,))
    t = near[:, None] + (far - near)[:, None] * np.linspace(0.0, 1.0, n_march)[None, :]
    sig = sigma64((o[:, None, :] + t[:, :, None] * d[:, None, :]).reshape(-1, 3)).reshape(R, n_march)
    ins = sig >= level
    cross = ~ins[:, :-1] & ins[:, 1:]
    has = cross.any(axis=1)
    state = np.where(ins[:, 0], 2, np.where(has, 1, 0)).astype(np.uint8)
    k = np.where(has, cross.argmax(axis=1), 0)
    rows = np.arange(R)
    lo, hi = t[rows, k].copy(), t[rows, k + 1].copy()
    hit = np.nonzero(state == 1)[0]
    for _ in range(n_bisect):
        mid = 0.5 * (lo[hit] + hi[hit])
        m_in = sigma64(o[hit] + mid[:, None] * d[hit]) >= level
        hi[hit] = np.where(m_in, mid, hi[hit])
        lo[hit] = np.where(m_in, lo[hit], mid)
    depth = np.where(state == 1, 0.5 * (lo + hi), np.where(state == 2, near, 0.0))
    return state, depth
