"""Test helper: a numpy restatement of the iso-surface backward of include/supnerf_hip.h ("Iso-surface backward") and
sup-nerf_amd/csrc/snr_iso_grad.hip, on top of tests/iso_restatement.py's forward.

Same fp32 operation sequence and the same gather order as the kernels, so that their output can be compared with ``np.array_equal``:
  * a vertex on crossing edge (u, d), va = f(u), vb = f(u + d): s = 0 + g_a h_a + ... over the axes a with d_a = 1 in axis order,
    w = s / ((vb - va) (vb - va)), terms w (level - vb) for u and w (va - level) for u + d;
  * every grid point sums acc = 0 + term + ... in fp32 over 14 slots in this order: outgoing d = 0..6 (its own edge bits), then incoming
    d = 0..6 (bit d of u - dir(d));
  * on_surface: 1 iff the point is an end of a crossing edge;
  * the surface points of each object in grid order, padded per object to n = the largest count rounded up to a multiple of 64 with
    (lo, 0).
Empty slots add +0, which changes no fp32 sum that starts at +0: the vectorised form below is the per-point loop of ``grid_grad_loop``.
"""
import numpy as np

from iso_restatement import DIR_BITS


def _offset(bits, n1, n2):
    return (bits & 1) * n1 * n2 + (bits >> 1 & 1) * n2 + (bits >> 2 & 1)


def edge_masks(f, level):
    """(n0, n1, n2) uint8 crossing-edge bits of every grid point, as snr_iso_count writes them."""
    f = np.asarray(f, dtype=np.float32)
    n0, n1, n2 = f.shape
    inside = f > np.float32(level)
    mask = np.zeros(f.shape, dtype=np.uint8)
    for d, bits in enumerate(DIR_BITS):
        dx, dy, dz = bits & 1, bits >> 1 & 1, bits >> 2 & 1
        a = inside[:n0 - dx, :n1 - dy, :n2 - dz]
        b = inside[dx:, dy:, dz:]
        mask[:n0 - dx, :n1 - dy, :n2 - dz] |= ((a != b).astype(np.uint8) << d)
    return mask


def vertex_edges(f, level):
    """(u, d) of every vertex of ``iso_restatement.extract(f, level)``, in its order (edge id 7 u + d)."""
    m = edge_masks(f, level).reshape(-1)
    u, d = np.nonzero((m[:, None] >> np.arange(7, dtype=np.uint8)[None, :]) & 1)     # row-major: ids 7 u + d in increasing order
    return u.astype(np.int64), d.astype(np.int64)


def vertex_weights(f, level, h, d_verts):
    """(u, d, w) per vertex: w = s / ((vb - va) (vb - va)) in fp32."""
    f = np.asarray(f, dtype=np.float32)
    n0, n1, n2 = f.shape
    h = np.asarray(h, dtype=np.float32)
    g = np.asarray(d_verts, dtype=np.float32).reshape(-1, 3)
    u, d = vertex_edges(f, level)
    assert g.shape[0] == u.shape[0]
    bits = np.array(DIR_BITS, dtype=np.int64)[d]
    ff = f.reshape(-1)
    va, vb = ff[u], ff[u + _offset(bits, n1, n2)]
    s = np.zeros(u.shape, dtype=np.float32)
    for a in range(3):
        on = (bits >> a & 1).astype(bool)
        s = np.where(on, s + g[:, a] * h[a], s).astype(np.float32)
    diff = (vb - va).astype(np.float32)
    w = (s / (diff * diff)).astype(np.float32)
    return u, d, w


def grid_grad(f, level, h, d_verts):
    """(d_grid (n0, n1, n2) fp32, on_surface (n0, n1, n2) uint8): the kernel's gather, vectorised over grid points."""
    f = np.asarray(f, dtype=np.float32)
    n0, n1, n2 = f.shape
    level = np.float32(level)
    ff = f.reshape(-1)
    nv = ff.shape[0]
    u, d, w = vertex_weights(f, level, h, d_verts)
    W = np.zeros((7, nv), dtype=np.float32)
    P = np.zeros((7, nv), dtype=bool)
    W[d, u] = w
    P[d, u] = True
    idx = np.arange(nv, dtype=np.int64)
    i, j, k = idx // (n1 * n2), idx // n2 % n1, idx % n2
    acc = np.zeros(nv, dtype=np.float32)
    on = np.zeros(nv, dtype=bool)
    for dd, bits in enumerate(DIR_BITS):                            # outgoing: this point is u
        off = _offset(bits, n1, n2)
        p = P[dd]
        vb = ff[np.minimum(idx + off, nv - 1)]
        acc = np.where(p, acc + W[dd] * (level - vb), acc).astype(np.float32)
        on |= p
    for dd, bits in enumerate(DIR_BITS):                            # incoming: this point is u + dir(d)
        off = _offset(bits, n1, n2)
        ok = (i >= (bits & 1)) & (j >= (bits >> 1 & 1)) & (k >= (bits >> 2 & 1))
        src = np.where(ok, idx - off, 0)
        p = ok & P[dd][src]
        va = ff[src]
        acc = np.where(p, acc + W[dd][src] * (va - level), acc).astype(np.float32)
        on |= p
    return acc.reshape(f.shape), on.astype(np.uint8).reshape(f.shape)


def grid_grad_loop(f, level, h, d_verts):
    """The same gather written as the kernel's per-point loop (slow: small grids only)."""
    f = np.asarray(f, dtype=np.float32)
    n0, n1, n2 = f.shape
    level = np.float32(level)
    h = np.asarray(h, dtype=np.float32)
    g = np.asarray(d_verts, dtype=np.float32).reshape(-1, 3)
    ff = f.reshape(-1)
    m = edge_masks(f, level).reshape(-1)
    base = np.cumsum([bin(int(x)).count("1") for x in m]) if m.size else np.zeros(0, dtype=np.int64)

    def weight(vid, bits, va, vb):
        s = np.float32(0)
        for a in range(3):
            if bits >> a & 1:
                s = np.float32(s + np.float32(g[vid, a] * h[a]))
        diff = np.float32(vb - va)
        return np.float32(s / np.float32(diff * diff))

    out = np.zeros(ff.shape, dtype=np.float32)
    for v in range(ff.shape[0]):
        i, j, k = v // (n1 * n2), v // n2 % n1, v % n2
        acc = np.float32(0)
        mv = int(m[v])
        w = int(base[v]) - bin(mv).count("1")
        for d, bits in enumerate(DIR_BITS):
            if mv >> d & 1:
                vb = ff[v + _offset(bits, n1, n2)]
                acc = np.float32(acc + np.float32(weight(w, bits, ff[v], vb) * np.float32(level - vb)))
                w += 1
        for d, bits in enumerate(DIR_BITS):
            if i < (bits & 1) or j < (bits >> 1 & 1) or k < (bits >> 2 & 1):
                continue
            p = v - _offset(bits, n1, n2)
            mp = int(m[p])
            if not mp >> d & 1:
                continue
            vid = int(base[p]) - bin(mp).count("1") + bin(mp & ((1 << d) - 1)).count("1")
            acc = np.float32(acc + np.float32(weight(vid, bits, ff[p], ff[v]) * np.float32(ff[p] - level)))
        out[v] = acc
    return out.reshape(f.shape)


def surface_points(on_surface, d_grid, lo, h):
    """on_surface, d_grid (B, n0, n1, n2) -> (xyz (B n, 3) fp32, d_sig (B n) fp32, n, counts (B,)), as snr_iso_surface_points writes
    them for n = the largest count rounded up to a multiple of 64."""
    on = np.asarray(on_surface).astype(bool)
    dg = np.asarray(d_grid, dtype=np.float32)
    B, n0, n1, n2 = on.shape
    lo, h = np.asarray(lo, dtype=np.float32), np.asarray(h, dtype=np.float32)
    counts = on.reshape(B, -1).sum(1)
    n = int(-(-int(counts.max()) // 64) * 64) if B else 0
    xyz = np.broadcast_to(lo, (B, n, 3)).astype(np.float32).copy()
    ds = np.zeros((B, n), dtype=np.float32)
    for b in range(B):
        v = np.nonzero(on[b].reshape(-1))[0]
        ijk = np.stack([v // (n1 * n2), v // n2 % n1, v % n2], axis=1).astype(np.float32)
        xyz[b, :v.size] = (lo[None, :] + h[None, :] * ijk).astype(np.float32)
        ds[b, :v.size] = dg[b].reshape(-1)[v]
    return xyz.reshape(B * n, 3), ds.reshape(B * n), n, counts


def vertices64(f, u, d, level, lo, h):
    """The vertex formula over a fixed edge list in the array library of ``f`` (numpy or torch, any float dtype): the function whose
    derivative the backward is."""
    import torch
    is_t = torch.is_tensor(f)
    n0, n1, n2 = f.shape
    bits = np.array(DIR_BITS, dtype=np.int64)[np.asarray(d)]
    off = _offset(bits, n1, n2)
    u = np.asarray(u)
    ff = f.reshape(-1)
    if is_t:
        ui, wi = torch.as_tensor(u), torch.as_tensor(u + off)
        va, vb = ff[ui], ff[wi]
    else:
        va, vb = ff[u], ff[u + off]
    t = (level - va) / (vb - va)
    ijk = np.stack([u // (n1 * n2), u // n2 % n1, u % n2], axis=1).astype(np.float64)
    dv = np.stack([bits & 1, bits >> 1 & 1, bits >> 2 & 1], axis=1).astype(np.float64)
    lo64, h64 = np.asarray(lo, dtype=np.float64), np.asarray(h, dtype=np.float64)
    if is_t:
        cast = lambda a: torch.as_tensor(a, dtype=f.dtype)            # noqa: E731
        return cast(lo64)[None, :] + cast(h64)[None, :] * (cast(ijk) + t[:, None] * cast(dv))
    return lo64[None, :] + h64[None, :] * (ijk + t[:, None] * dv)
