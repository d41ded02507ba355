"""Test helper: a numpy restatement of the iso-surface rules of include/supnerf_hip.h ("Geometry") and sup-nerf_amd/csrc/snr_iso.hip.

Same order, same fp32 operation sequence, same quad split and same winding, so that the kernels' vertex and face arrays can be compared
with ``np.array_equal``.  Written for clarity over speed (vectorised over cells, looped over the 6 tetrahedra), like ``relu_bits.py``.

Rules:
  * inside iff value > level (fp32);
  * grid vertex u = (i n1 + j) n2 + k; edge (u, d), d = 0..6 for x, y, z, xy, xz, yz, xyz (corner bits 1, 2, 4, 3, 5, 6, 7); id 7 u + d;
  * one vertex per crossing edge in id order: t = (level - f(u)) / (f(u + d) - f(u)), c_a = lo_a + h_a (i_a + t d_a), each step in fp32;
  * cell corners v000 + bits; tetrahedra v000 -> +e_a -> +e_a+e_b -> v111 for (a, b, c) in 012, 021, 102, 120, 201, 210, positive for the
    even permutations;
  * 1 (or 3) inside: the lone vertex i and the even permutation (i, j, k, l) -> triangle (ij, ik, il), second and third swapped unless
    "positive" == "one inside";
  * 2 inside {i, j}: the even permutation (i, j, k, l) -> quad (ik, il, jl, jk), reversed to (ik, jk, jl, il) on a negative tetrahedron,
    split at its vertex m of smallest edge id into (m, m+1, m+2), (m, m+2, m+3);
  * faces in the order cell, tetrahedron, triangle.
"""
import numpy as np

DIR_BITS = (1, 2, 4, 3, 5, 6, 7)
DIR_OF = {b: d for d, b in enumerate(DIR_BITS)}
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
POSITIVE = (True, False, False, True, True, False)
EVEN1 = ((0, 1, 2, 3), (1, 0, 3, 2), (2, 0, 1, 3), (3, 0, 2, 1))
EVEN2 = {3: (0, 1, 2, 3), 5: (0, 2, 3, 1), 6: (1, 2, 0, 3), 9: (0, 3, 1, 2), 10: (1, 3, 2, 0), 12: (2, 3, 0, 1)}


def _parity_even(p):
    p = list(p)
    inv = sum(1 for a in range(4) for b in range(a + 1, 4) if p[a] > p[b])
    return inv % 2 == 0


assert all(_parity_even(e) and e[0] == i for i, e in enumerate(EVEN1))
assert all(_parity_even(e) and {e[0], e[1]} == {p for p in range(4) if s >> p & 1} and e[0] < e[1] for s, e in EVEN2.items())


def _case_triangles(s, pos):
    """Triangles of one tetrahedron case as lists of tetrahedron-vertex pairs; a quad is returned as ("quad", 4 pairs)."""
    n = bin(s).count("1")
    if n in (1, 3):
        x = s if n == 1 else (~s & 15)          # the lone vertex: the one inside (n = 1) or the one outside (n = 3)
        lone = x.bit_length() - 1
        i, j, k, l = EVEN1[lone]
        keep = pos == (n == 1)
        return ("tri", [(i, j), (i, k), (i, l)] if keep else [(i, j), (i, l), (i, k)])
    if n == 2:
        i, j, k, l = EVEN2[s]
        q = [(i, k), (i, l), (j, l), (j, k)]
        if not pos:
            q = [q[0], q[3], q[2], q[1]]
        return ("quad", q)
    return (None, [])


def extract(field, level, lo=(0.0, 0.0, 0.0), h=(1.0, 1.0, 1.0)):
    """field (n0, n1, n2) -> verts (V, 3) float32, faces (F, 3) int32, as snr_iso_count / snr_iso_emit compute them for one object."""
    f = np.ascontiguousarray(field, dtype=np.float32)
    n0, n1, n2 = f.shape
    level = np.float32(level)
    lo = np.asarray(lo, dtype=np.float32)
    h = np.asarray(h, dtype=np.float32)
    inside = f > level
    nv = n0 * n1 * n2
    idx = np.arange(nv, dtype=np.int64).reshape(n0, n1, n2)

    # crossing edges, one bit per direction at the lower endpoint
    mask = np.zeros((n0, n1, n2), dtype=np.uint8)
    for d, bits in enumerate(DIR_BITS):
        dx, dy, dz = bits & 1, bits >> 1 & 1, bits >> 2 & 1
        a = inside[:n0 - dx, :n1 - dy, :n2 - dz]
        b = inside[dx:, dy:, dz:]
        mask[:n0 - dx, :n1 - dy, :n2 - dz] |= ((a != b).astype(np.uint8) << d)
    flat_mask = mask.reshape(-1)
    popc = np.unpackbits(flat_mask[:, None], axis=1).sum(1).astype(np.int64)
    base = np.cumsum(popc) - popc                       # exclusive scan: index of the grid vertex's first vertex

    # vertices in edge-id order
    us, ds = [], []
    for d in range(7):
        sel = np.nonzero(flat_mask >> d & 1)[0]
        us.append(sel)
        ds.append(np.full(sel.shape, d, dtype=np.int64))
    u = np.concatenate(us)
    d = np.concatenate(ds)
    order = np.argsort(7 * u + d, kind="stable")
    u, d = u[order], d[order]
    bits = np.array(DIR_BITS, dtype=np.int64)[d]
    off = (bits & 1) * n1 * n2 + (bits >> 1 & 1) * n2 + (bits >> 2 & 1)
    ff = f.reshape(-1)
    va, vb = ff[u], ff[u + off]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (level - va) / (vb - va)
    ijk = np.stack([u // (n1 * n2), u // n2 % n1, u % n2], axis=1).astype(np.float32)
    dvec = np.stack([bits & 1, bits >> 1 & 1, bits >> 2 & 1], axis=1).astype(np.float32)
    verts = lo[None, :] + h[None, :] * (ijk + t[:, None] * dvec)
    verts = verts.astype(np.float32)

    # faces, cell by cell (vectorised over cells), tetrahedron by tetrahedron
    if min(n0, n1, n2) < 2:
        return verts, np.zeros((0, 3), dtype=np.int32)
    v0 = idx[:-1, :-1, :-1].reshape(-1)
    nc = v0.shape[0]

    def corner_off(c):
        return (c & 1) * n1 * n2 + (c >> 1 & 1) * n2 + (c >> 2 & 1)

    ins = ff[v0[:, None] + np.array([corner_off(c) for c in range(8)])[None, :]] > level      # (nc, 8)
    out_f = np.full((nc, 6, 2, 3), -1, dtype=np.int64)
    valid = np.zeros((nc, 6, 2), dtype=bool)
    for t_i, (a, b, _) in enumerate(PERMS):
        corner = (0, 1 << a, (1 << a) | (1 << b), 7)
        s = sum(ins[:, corner[p]].astype(np.int64) << p for p in range(4))

        def edge(p, q):
            p, q = min(p, q), max(p, q)
            uu = v0 + corner_off(corner[p])
            dd = DIR_OF[corner[q] ^ corner[p]]
            m = flat_mask[uu].astype(np.int64)
            vid = base[uu] + np.unpackbits((m & ((1 << dd) - 1)).astype(np.uint8)[:, None], axis=1).sum(1)
            return 7 * uu + dd, vid

        for sv in range(1, 15):
            cells = np.nonzero(s == sv)[0]
            if cells.size == 0:
                continue
            kind, pairs = _case_triangles(sv, POSITIVE[t_i])
            ev = [edge(p, q) for p, q in pairs]
            ids = np.stack([e[0][cells] for e in ev], axis=1)
            vids = np.stack([e[1][cells] for e in ev], axis=1)
            if kind == "tri":
                out_f[cells, t_i, 0] = vids
                valid[cells, t_i, 0] = True
            else:
                m = np.argmin(ids, axis=1)
                r = np.arange(cells.size)
                q = [vids[r, (m + k) % 4] for k in range(4)]
                out_f[cells, t_i, 0] = np.stack([q[0], q[1], q[2]], axis=1)
                out_f[cells, t_i, 1] = np.stack([q[0], q[2], q[3]], axis=1)
                valid[cells, t_i, :] = True
    faces = out_f[valid].astype(np.int32)
    return verts, faces


def extract_batch(fields, level, lo=(0.0, 0.0, 0.0), h=(1.0, 1.0, 1.0)):
    return [extract(f, level, lo, h) for f in fields]


# ---------------------------------------------------------------------------------------------------------------- mesh measures
def edge_use(faces):
    """{undirected edge: number of faces using it}, and whether every directed edge occurs once (consistent orientation)."""
    f = np.asarray(faces, dtype=np.int64)
    directed = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    und = np.sort(directed, axis=1)
    _, cnt = np.unique(und, axis=0, return_counts=True)
    _, dcnt = np.unique(directed, axis=0, return_counts=True)
    return cnt, bool((dcnt == 1).all())


def euler_characteristic(verts, faces):
    f = np.asarray(faces, dtype=np.int64)
    used = np.unique(f)
    und = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1), axis=0)
    return used.size - und.shape[0] + f.shape[0]


def signed_volume(verts, faces):
    v = np.asarray(verts, dtype=np.float64)[np.asarray(faces, dtype=np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def area(verts, faces):
    v = np.asarray(verts, dtype=np.float64)[np.asarray(faces, dtype=np.int64)]
    return float(np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1).sum() / 2.0)


def read_ply(path):
    """Binary little-endian PLY with float x, y, z vertices and int32-indexed triangle lists -> (verts (V,3) float32, faces (F,3) int32)."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode("ascii").splitlines()
    assert header[0] == "ply" and header[1] == "format binary_little_endian 1.0", header[:2]
    nv = nf = 0
    for line in header:
        if line.startswith("element vertex"):
            nv = int(line.split()[-1])
        elif line.startswith("element face"):
            nf = int(line.split()[-1])
    verts = np.frombuffer(data, dtype="<f4", count=3 * nv, offset=end).reshape(nv, 3)
    rec = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    faces = np.frombuffer(data, dtype=rec, count=nf, offset=end + 12 * nv)
    assert (faces["n"] == 3).all()
    assert end + 12 * nv + 13 * nf == len(data)
    return verts.copy(), faces["i"].astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- analytic fields
def lattice(n, lo, hi):
    """Per-axis lo, h and the fp32 coordinates lo + h i (one multiply, one add), as the kernels make them."""
    n = np.broadcast_to(np.asarray(n), (3,)).astype(np.int64)
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float32), (3,)).astype(np.float32)
    hi = np.broadcast_to(np.asarray(hi, dtype=np.float32), (3,)).astype(np.float32)
    h = ((hi - lo) / np.maximum(n - 1, 1).astype(np.float32)).astype(np.float32)
    axes = [(lo[a] + h[a] * np.arange(n[a], dtype=np.float32)).astype(np.float32) for a in range(3)]
    return lo, h, axes


def sphere_field(n, r=0.35, lo=-0.5, hi=0.5):
    """r^2 - |x|^2 (positive inside) on an n^3 lattice; level 0."""
    lo, h, (x, y, z) = lattice(n, lo, hi)
    X, Y, Z = np.meshgrid(x, y, z, indexing="ij")
    return (np.float32(r * r) - (X * X + Y * Y + Z * Z)).astype(np.float32), lo, h


def torus_field(n, R=0.3, r=0.1, lo=-0.5, hi=0.5):
    lo, h, (x, y, z) = lattice(n, lo, hi)
    X, Y, Z = np.meshgrid(x, y, z, indexing="ij")
    q = np.sqrt(X * X + Y * Y) - np.float32(R)
    return (np.float32(r * r) - (q * q + Z * Z)).astype(np.float32), lo, h


def noise_field(n, seed=0):
    """A smooth random field with many components (sum of random plane waves) -- many small closed pieces and holes."""
    rng = np.random.default_rng(seed)
    lo, h, (x, y, z) = lattice(n, -0.5, 0.5)
    X, Y, Z = np.meshgrid(x, y, z, indexing="ij")
    acc = np.zeros_like(X, dtype=np.float64)
    for _ in range(12):
        k = rng.normal(size=3) * 14.0
        acc += np.cos(k[0] * X + k[1] * Y + k[2] * Z + rng.uniform(0, 2 * np.pi))
    return (acc / 12.0).astype(np.float32), lo, h


def level_equal_field(n):
    """Integer-valued field with many samples exactly at level 0 (ties count as outside)."""
    lo, h, _ = lattice(n, -0.5, 0.5)
    i, j, k = np.meshgrid(*[np.arange(n)] * 3, indexing="ij")
    return (((i * 7 + j * 3 + k * 5) % 5) - 2).astype(np.float32) * np.float32(0.5) * ((i + j + k) % 2).astype(np.float32), lo, h
