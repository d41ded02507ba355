"""The rules of include/supnerf_hip.h ("Mesh painting") restated in numpy: one plain function per rule P1 - P6, no kernel code.  Every fp32
step is ONE numpy float32 operation on float32 operands (one rounding), in the order the header writes it; the only float64 arithmetic
is where rule P6 says float64.  The GPU tests compare the package against it bit for bit; the CPU tests hold the restatement itself
against results worked out by hand.  ``planted`` switches in a deliberate mistake, so that the checks can be shown to reject one.

``colour64`` is the float64 "what it should be" evaluator of P1 / P2 for the analytic cases: the same taps and validity, every product,
sum and the division in float64."""
import numpy as np

F32 = np.float32
PLANTED = ("no_depth_test", "all_taps", "half_pixel", "nearest", "descending", "tie_high")
TAPS = ((0, 0), (1, 0), (0, 1), (1, 1))              # (dx, dy) in the order of rule P1


def _f32(a):
    return np.ascontiguousarray(a, F32)


# ------------------------------------------------------------------ P1
def _axis(u, n, planted=None):
    """One axis of P1: (inside, i0 int64, t fp32 = the weight of the upper tap)."""
    u = _f32(u)
    if planted == "half_pixel":
        u = u - F32(0.5)                                  # the usual mistake: pixel centres at half-integers
    with np.errstate(all="ignore"):
        inside = ~((u < F32(0)) | (u > F32(n - 1))) & np.isfinite(u)
        safe = np.where(inside, u, F32(0))
        if n == 1:
            return inside, np.zeros(u.shape, np.int64), np.zeros(u.shape, F32)
        if planted == "nearest":
            i = np.rint(safe).astype(np.int64)
            i0 = np.minimum(i, n - 2)
            return inside, i0, (i - i0).astype(F32)       # weight 1 on the nearest pixel, 0 on the other
        i0 = np.minimum(np.floor(safe).astype(np.int64), n - 2)
        return inside, i0, (safe - i0.astype(F32)).astype(F32)


def footprint(screen, H, W, z_near, planted=None):
    """P1: dict(inside (V,) bool, tap (V, 4) int64 = the pixel index y W + x of each tap in tap order, -1 for the duplicate of a tap when
    W or H is 1, weight (V, 4) fp32)."""
    screen = _f32(screen).reshape(-1, 3)
    z = screen[:, 2]
    with np.errstate(all="ignore"):
        in_x, x0, a = _axis(screen[:, 0], W, planted)
        in_y, y0, b = _axis(screen[:, 1], H, planted)
        inside = in_x & in_y & np.isfinite(z) & ~(z < F32(z_near))
        wx, wy = (F32(1) - a, a), (F32(1) - b, b)
        tap = np.stack([(y0 + dy) * W + (x0 + dx) for dx, dy in TAPS], axis=1)
        weight = np.stack([wx[dx] * wy[dy] for dx, dy in TAPS], axis=1).astype(F32)
    for t, (dx, dy) in enumerate(TAPS):
        if (dx and W == 1) or (dy and H == 1):
            tap[:, t] = -1
    tap[~inside] = -1
    return dict(inside=inside, tap=tap, weight=weight)


# ------------------------------------------------------------------ P2
def valid_taps(z, tap, depth, mask, tol, planted=None):
    """P2: (V, 4) bool."""
    d = _f32(depth).reshape(-1)
    exists = tap >= 0
    q = np.where(exists, tap, 0)
    with np.errstate(all="ignore"):
        ok = exists & (d[q] > F32(0))
        if mask is not None:
            ok &= _f32(mask).reshape(-1)[q] > F32(0)
        if planted != "no_depth_test":
            ok &= _f32(z)[:, None] <= d[q] + F32(tol)
    if planted == "all_taps":
        ok = exists
    return ok


def view_colour(fp, valid, image):
    """P2: (s (V,) fp32, c (V, 3) fp32): the sums run over the valid taps in tap order, starting from the first valid term; c is
    divided by s where s > 0 (and means nothing elsewhere)."""
    img = _f32(image).reshape(-1, 3)
    V = valid.shape[0]
    s, c, started = np.zeros(V, F32), np.zeros((V, 3), F32), np.zeros(V, bool)
    with np.errstate(all="ignore"):
        for t in range(4):
            v = valid[:, t]
            w = fp["weight"][:, t]
            term = w[:, None] * img[np.where(v, fp["tap"][:, t], 0)]
            s = np.where(v, np.where(started, s + w, w), s).astype(F32)
            c = np.where(v[:, None], np.where(started[:, None], c + term, term), c).astype(F32)
            started |= v
        seen = s > F32(0)
        c = np.where(seen[:, None], c / np.where(seen, s, F32(1))[:, None], c).astype(F32)
    return s, c


def colour64(screen, image, mask, depth, tol, z_near=1e-3):
    """The float64 evaluator: (seen (V,) bool, c (V, 3) float64) of P1 / P2 with exact taps and every operation in float64."""
    H, W = np.shape(depth)
    fp = footprint(screen, H, W, z_near)
    valid = valid_taps(_f32(screen).reshape(-1, 3)[:, 2], fp["tap"], depth, mask, tol)
    u, v = _f32(screen).reshape(-1, 3)[:, 0].astype(np.float64), _f32(screen).reshape(-1, 3)[:, 1].astype(np.float64)
    x0 = np.zeros_like(u) if W == 1 else np.minimum(np.floor(np.where(fp["inside"], u, 0)), W - 2)
    y0 = np.zeros_like(v) if H == 1 else np.minimum(np.floor(np.where(fp["inside"], v, 0)), H - 2)
    a, b = (u - x0 if W > 1 else 0 * u), (v - y0 if H > 1 else 0 * v)
    w = np.stack([(1 - a) * (1 - b), a * (1 - b), (1 - a) * b, a * b], axis=1) * valid
    img = np.asarray(image, np.float64).reshape(-1, 3)
    s = w.sum(1)
    num = (w[:, :, None] * img[np.where(valid, fp["tap"], 0)]).sum(1)
    seen = fp["inside"] & (s > 0)
    return seen, num / np.where(seen, s, 1.0)[:, None]


# ------------------------------------------------------------------ P3
def facing(verts, normals, centre):
    """P3: g (V,) fp32; all ones without normals."""
    x = _f32(verts).reshape(-1, 3)
    if normals is None:
        return np.ones(x.shape[0], F32)
    n, c = _f32(normals).reshape(-1, 3), [F32(v) for v in centre]
    with np.errstate(all="ignore"):
        d = [c[k] - x[:, k] for k in range(3)]
        dot = (n[:, 0] * d[0] + n[:, 1] * d[1]) + n[:, 2] * d[2]
        nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        den = nn * dd
        ok = (dot > F32(0)) & (den > F32(0)) & (den < F32(np.inf))
        return np.where(ok, (dot * dot) / np.where(ok, den, F32(1)), F32(0)).astype(F32)


# ------------------------------------------------------------------ P4
def new_state(n):
    return dict(sum_rgb=np.zeros((n, 3), F32), sum_w=np.zeros(n, F32), seen=np.zeros(n, np.int32), best_w=np.zeros(n, F32),
                best=np.full(n, -1, np.int32), best_rgb=np.zeros((n, 3), F32))


def accumulate(state, sees, g, c, k, planted=None):
    """P4, in place: the vertices ``sees`` marks take view k's colour c with weight g."""
    with np.errstate(all="ignore"):
        i = np.nonzero(sees)[0]
        state["sum_rgb"][i] = state["sum_rgb"][i] + g[i, None] * c[i]
        state["sum_w"][i] = state["sum_w"][i] + g[i]
        state["seen"][i] += 1
        better = (g[i] >= state["best_w"][i]) if planted == "tie_high" else (g[i] > state["best_w"][i])
        j = i[better]
        state["best_w"][j], state["best"][j], state["best_rgb"][j] = g[j], k, c[j]
    return state


def paint_view(screen, verts, normals, image, mask, depth, centre, tol, z_near, k, state, planted=None):
    """P1 - P4 for one view: ``snr_paint_view``.  Returns dict(sees, g, s, c) of this view beside the updated ``state``."""
    H, W = np.shape(depth)
    V = np.shape(screen)[0]
    if H == 0 or W == 0 or V == 0:
        return dict(sees=np.zeros(V, bool), g=np.zeros(V, F32), s=np.zeros(V, F32), c=np.zeros((V, 3), F32))
    fp = footprint(screen, H, W, z_near, planted)
    valid = valid_taps(_f32(screen).reshape(-1, 3)[:, 2], fp["tap"], depth, mask, tol, planted)
    s, c = view_colour(fp, valid, image)
    g = facing(verts, normals, centre) if normals is not None else np.ones(V, F32)
    with np.errstate(all="ignore"):
        sees = fp["inside"] & (g > F32(0)) & (s > F32(0))
    accumulate(state, sees, g, c, k, planted)
    return dict(sees=sees, g=g, s=s, c=c)


# ------------------------------------------------------------------ P5
def finish(state, blend, background=0.0):
    """P5: (colors (V, 3) fp32, filled (V,) int32); ``blend`` 0 / "weighted" or 1 / "best"."""
    best = blend in (1, "best")
    hit = state["seen"] > 0
    with np.errstate(all="ignore"):
        c = state["best_rgb"] if best else state["sum_rgb"] / np.where(hit, state["sum_w"], F32(1))[:, None]
    colors = np.where(hit[:, None], c, F32(background)).astype(F32)
    return colors, np.where(hit, 0, -1).astype(np.int32)


# ------------------------------------------------------------------ P6
def fill_round(colors, filled, adj, r):
    """P6, one Jacobi round r over ``smooth_restatement.adjacency`` of ONE object: new (colors, filled)."""
    colors, filled = _f32(colors), np.asarray(filled, np.int32)
    start, nbr, deg = adj["nbr_start"], adj["nbr"], adj["degree"]
    V = filled.shape[0]
    s, n = np.zeros((V, 3), np.float64), np.zeros(V, np.int64)
    for k in range(int(deg.max(initial=0))):                 # pass k adds every vertex's k-th neighbour: its own ascending order
        has = np.nonzero(deg > k)[0]
        j = nbr[start[has] + k]
        ok = filled[j] >= 0
        s[has[ok]] += colors[j[ok]].astype(np.float64)
        n[has[ok]] += 1
    take = (filled < 0) & (n > 0)
    out, out_f = colors.copy(), filled.copy()
    out[take] = (s[take] / n[take, None].astype(np.float64)).astype(F32)
    out_f[take] = r
    return out, out_f


def fill(colors, filled, adj, rounds):
    colors, filled = _f32(colors).copy(), np.asarray(filled, np.int32).copy()
    for r in range(1, rounds + 1):
        colors, filled = fill_round(colors, filled, adj, r)
    return colors, filled


# ------------------------------------------------------------------ the chain
def paint(verts, normals, views, blend="weighted", background=0.0, z_near=1e-3, rounds=0, adj=None, fallback=None, planted=None):
    """``paint_mesh`` after the rasteriser: ``views`` = [dict(screen, depth, image, mask or None, centre, tol)] in ascending order.
    Returns dict(colors, weight, seen, best, filled, state)."""
    V = np.shape(verts)[0]
    state = new_state(V)
    order = list(enumerate(views))
    if planted == "descending":
        order.reverse()
    for k, v in order:
        paint_view(v["screen"], verts, normals, v["image"], v.get("mask"), v["depth"], v["centre"], v["tol"], z_near, k, state, planted)
    colors, filled = finish(state, blend, background)
    if rounds:
        colors, filled = fill(colors, filled, adj, rounds)
    if fallback is not None:
        colors = np.where((filled < 0)[:, None], _f32(fallback), colors)
    return dict(colors=colors, weight=state["best_w"] if blend in (1, "best") else state["sum_w"], seen=state["seen"], best=state["best"],
                filled=filled, state=state)
