"""Test helper: a numpy restatement of the mesh-component rules of include/supnerf_hip.h ("Mesh components") and
sup-nerf_amd/csrc/snr_mesh.hip, for one object: verts (V, 3) float32, faces (F, 3) int32.

Written for clarity over speed, like ``iso_restatement.py``: no union-find, no atomics -- every vertex simply ends up knowing the smallest
vertex index it can reach.

Rules:
  1. two vertices are connected iff a chain of faces links them through shared vertex INDICES (equal positions do not connect; a vertex no
     face names is a component of its own with 0 faces);
  2. component c is the one whose smallest vertex index is the c-th smallest among the object's components; vert_label (V,) int32,
     face_label (F,) int32 = the label of the face's first vertex;
  3. per component: n_verts, n_faces (int64); bbox_lo, bbox_hi (C, 3) float32 = min / max of its vertex coordinates; area and volume in
     float64: with a, b, c the face's vertices widened to float64 and p0 the component's vertex of smallest index,
     area term = |(b - a) x (c - a)| / 2, volume term = (a - p0) . ((b - p0) x (c - p0)) / 6, summed over the component's faces.  The
     order is fixed: the terms as ``face_terms_exact`` writes them out, the faces sorted by component with a stable sort, then the header's
     "Fixed-order segmented sums" -- ``components_fixed_order`` restates it and is compared bit for bit.  ``components`` sums in face order
     with numpy's own term order; the two, and the device, lie within ``sum_bounds`` of each other, which is still asserted;
  4. a subset of components gives a sub-mesh: the kept vertices and faces in their original order, indices renumbered, with the index
     maps into the original arrays.

Also here: one step function per kernel of snr_mesh.hip (``roots_of``, ``labels_from``, ``boxes_from``, ``face_terms_exact``) for the
tests that drive the kernels alone, the policy of ``geometry.largest_component`` restated on these arrays, and the analytic grids the tests
share."""
import numpy as np

import segment_sum_restatement as SS


def reach_smallest(n_verts, faces):
    """(V,) int64: for every vertex the smallest vertex index connected to it (rule 1).  Repeats two steps until nothing changes: every
    vertex of a face takes the smallest value the face's three vertices hold; every vertex takes the value held by the vertex it
    points at."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= n_verts):
        raise ValueError("a face index lies outside the mesh")
    low = np.arange(n_verts, dtype=np.int64)
    while True:
        new = low.copy()
        if f.size:
            np.minimum.at(new, f.reshape(-1), np.repeat(new[f].min(axis=1), 3))
        while True:
            hop = new[new]
            if np.array_equal(hop, new):
                break
            new = hop
        if np.array_equal(new, low):
            return low
        low = new


def labels(n_verts, faces):
    """Rule 2: (vert_label (V,) int32, face_label (F,) int32, first (C,) int64 = the smallest vertex index of every component)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    low = reach_smallest(n_verts, f)
    first = np.unique(low)                                      # ascending: position = component id
    vert_label = np.searchsorted(first, low).astype(np.int32)
    face_label = vert_label[f[:, 0]].astype(np.int32) if f.size else np.zeros(0, np.int32)
    return vert_label, face_label, first


def face_terms(verts, faces, p0):
    """Rule 3's two float64 terms per face, p0 (F, 3) the reference vertex of each face's component; and the magnitude
    |a - p0| |b - p0| |c - p0| / 6 that bounds the volume term's rounding."""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    area = np.linalg.norm(np.cross(b - a, c - a), axis=1) / 2.0
    a, b, c = a - p0, b - p0, c - p0
    vol = np.einsum("ij,ij->i", a, np.cross(b, c)) / 6.0
    mag = np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1) * np.linalg.norm(c, axis=1) / 6.0
    return area, vol, mag


def components(verts, faces):
    """Everything rule 2 and 3 define for one object, as a dict of numpy arrays (keys as ``geometry.Components``), plus ``first`` and the
    two magnitudes ``S_area``, ``S_volume`` of ``sum_bounds``."""
    verts = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V = verts.shape[0]
    vert_label, face_label, first = labels(V, f)
    C = first.shape[0]
    lo = np.full((C, 3), np.inf, np.float32)
    hi = np.full((C, 3), -np.inf, np.float32)
    for k in range(3):
        np.minimum.at(lo[:, k], vert_label, verts[:, k])
        np.maximum.at(hi[:, k], vert_label, verts[:, k])
    p0 = verts.astype(np.float64)[first[face_label]] if f.size else np.zeros((0, 3))
    area_t, vol_t, mag = face_terms(verts, f, p0)
    area, volume = np.zeros(C), np.zeros(C)
    np.add.at(area, face_label, area_t)
    np.add.at(volume, face_label, vol_t)
    return dict(vert_label=vert_label, face_label=face_label, first=first,
                n_verts=np.bincount(vert_label, minlength=C).astype(np.int64), n_faces=np.bincount(face_label, minlength=C).astype(np.int64),
                area=area, volume=volume, bbox_lo=lo, bbox_hi=hi, S_area=float(np.abs(area_t).sum()), S_volume=float(mag.sum()))


def face_terms_exact(verts, faces, p0):
    """Rule 3's two float64 terms per face in exactly the kernel's operation order (``mesh_face_terms_kernel``), every operation one IEEE
    float64 operation, written out elementwise: with e1 = b - a, e2 = c - a,
        n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x),     area = sqrt((nx nx + ny ny) + nz nz) / 2,
    and with a' = a - p0, b' = b - p0, c' = c - p0 and c = b' x c' formed the same way,
        volume = ((a'x cx + a'y cy) + a'z cz) / 6.
    ``p0`` (F, 3): the reference vertex of each face's component.  Returns (area (F,), volume (F,)) float64."""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    p = np.asarray(p0, dtype=np.float64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    e1x, e1y, e1z = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1], b[:, 2] - a[:, 2]
    e2x, e2y, e2z = c[:, 0] - a[:, 0], c[:, 1] - a[:, 1], c[:, 2] - a[:, 2]
    nx, ny, nz = e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x
    area = np.sqrt((nx * nx + ny * ny) + nz * nz) / 2.0
    ax, ay, az = a[:, 0] - p[:, 0], a[:, 1] - p[:, 1], a[:, 2] - p[:, 2]
    bx, by, bz = b[:, 0] - p[:, 0], b[:, 1] - p[:, 1], b[:, 2] - p[:, 2]
    cx, cy, cz = c[:, 0] - p[:, 0], c[:, 1] - p[:, 1], c[:, 2] - p[:, 2]
    ux, uy, uz = by * cz - bz * cy, bz * cx - bx * cz, bx * cy - by * cx
    return area, ((ax * ux + ay * uy) + az * uz) / 6.0


def components_fixed_order(verts, faces, comp=None):
    """``components`` with ``area`` and ``volume`` summed as the device sums them, bit for bit: the exact terms, sorted by ``face_label``
    with the stable argsort (ascending face order within a component), summed by ``segment_sum_restatement.segment_sum`` over
    ``segments(...)``.  ``comp``: what ``components`` gave for this mesh, to save computing it again."""
    verts = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    out = dict(components(verts, f) if comp is None else comp)
    C = out["first"].shape[0]
    p0 = verts.astype(np.float64)[out["first"][out["face_label"]]] if f.size else np.zeros((0, 3))
    area_t, vol_t = face_terms_exact(verts, f, p0)
    order, start, _ = SS.segments(out["face_label"], C)
    both = SS.segment_sum(np.stack([area_t, vol_t], axis=1)[order], start) if f.size else np.zeros((C, 2))
    out["area"], out["volume"] = both[:, 0].copy(), both[:, 1].copy()
    return out


# ---------------------------------------------------------------------------------------------------------------- one step per kernel
def roots_of(parent):
    """(V,) the root above every vertex of a forest ``parent`` (V,) with parent[i] <= i: follow the pointers until one points at itself.
    What ``snr_mesh_flatten`` must give for any such forest of one object (indices local to it)."""
    parent = np.asarray(parent, dtype=np.int64)
    root = np.arange(parent.shape[0], dtype=np.int64)
    while True:
        up = parent[root]
        if np.array_equal(up, root):
            return root.astype(np.int32)
        root = up


def labels_from(root, root_scan, faces, n_verts):
    """``snr_mesh_label`` for one object: vert_label[v] = root_scan[root[v]] - 1; face_label = the label of the face's first vertex, -1
    where that index lies outside [0, V) -- the other two indices play no part (rule 2)."""
    root, root_scan = np.asarray(root, dtype=np.int64), np.asarray(root_scan, dtype=np.int64)
    vert_label = (root_scan[root] - 1).astype(np.int32)
    i0 = np.asarray(faces, dtype=np.int64).reshape(-1, 3)[:, 0]
    ok = (i0 >= 0) & (i0 < n_verts)
    face_label = np.full(i0.shape[0], -1, np.int32)
    face_label[ok] = vert_label[i0[ok]]
    return vert_label, face_label


def boxes_from(verts, vert_label, n_comps):
    """``snr_mesh_boxes`` for one object: (comp_verts (C,) int64, bbox_lo, bbox_hi (C, 3) float32) over the vertices whose label lies in
    [0, n_comps); the others are not counted.  A component no vertex counts for keeps +inf / -inf here: its box is unspecified."""
    verts = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    lab = np.asarray(vert_label, dtype=np.int64)
    ok = (lab >= 0) & (lab < n_comps)
    lo = np.full((n_comps, 3), np.inf, np.float32)
    hi = np.full((n_comps, 3), -np.inf, np.float32)
    for k in range(3):
        np.minimum.at(lo[:, k], lab[ok], verts[ok, k])
        np.maximum.at(hi[:, k], lab[ok], verts[ok, k])
    return np.bincount(lab[ok], minlength=n_comps).astype(np.int64), lo, hi


def sum_bounds(comp):
    """What any float64 summation order may differ by from any other, plus the rounding of the terms themselves: (F + 16) 2^-52 S per
    object, S = sum |area term| for the area and sum |a - p0| |b - p0| |c - p0| / 6 for the volume.  (A sum of n float64 terms in any order
    is within (n - 1) 2^-53 sum |term| of the exact sum to first order, so two orders are within (n - 1) 2^-52 of each other; the 16 are
    room for the few roundings inside each term.)"""
    F = int(comp["face_label"].shape[0])
    return (F + 16) * 2.0 ** -52 * comp["S_area"], (F + 16) * 2.0 ** -52 * comp["S_volume"]


def select(verts, faces, comp, keep):
    """Rule 4: (verts, faces, vert_index, face_index) of the components ``keep`` (a bool mask (C,) or a list of ids)."""
    verts = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    C = comp["n_verts"].shape[0]
    mask = np.zeros(C, bool)
    keep = np.asarray(keep)
    if keep.dtype == bool:
        mask[:] = keep
    else:
        mask[keep.astype(np.int64)] = True
    vkeep, fkeep = mask[comp["vert_label"]], mask[comp["face_label"]]
    vert_index, face_index = np.nonzero(vkeep)[0], np.nonzero(fkeep)[0]
    renumber = np.cumsum(vkeep) - 1
    return verts[vert_index], renumber[f[face_index]].astype(np.int32).reshape(-1, 3), vert_index, face_index


def largest(comp, by="area", drop_cavities=True):
    """The mask of ``geometry.largest_component``: the component of most area / |volume| / faces (ties: the lowest id); with
    ``drop_cavities=False`` also every component of negative volume whose bounding box lies inside the winner's."""
    score = {"area": comp["area"], "volume": np.abs(comp["volume"]), "faces": comp["n_faces"]}[by]
    mask = np.zeros(score.shape[0], bool)
    if score.shape[0] == 0:
        return mask
    w = int(np.nonzero(score == score.max())[0][0])
    mask[w] = True
    if not drop_cavities:
        inside = (comp["bbox_lo"] >= comp["bbox_lo"][w]).all(1) & (comp["bbox_hi"] <= comp["bbox_hi"][w]).all(1)
        mask |= inside & (comp["volume"] < 0)
    return mask


def permuted(verts, faces, perm, face_order=None):
    """The same surface with vertex i renamed perm[i] (and the faces reordered by ``face_order``): what a caller's own mesh may look like."""
    verts = np.asarray(verts, dtype=np.float32)
    perm = np.asarray(perm, dtype=np.int64)
    out = np.empty_like(verts)
    out[perm] = verts
    f = perm[np.asarray(faces, dtype=np.int64)].astype(np.int32).reshape(-1, 3)
    return out, (f if face_order is None else f[np.asarray(face_order)])


# ---------------------------------------------------------------------------------------------------------------- analytic grids
def _lattice(n, lo=-0.5, hi=0.5):
    lo32, hi32 = np.float32(lo), np.float32(hi)
    h = (hi32 - lo32) / np.float32(n - 1)
    x = (lo32 + h * np.arange(n, dtype=np.float32)).astype(np.float32)
    return np.meshgrid(x, x, x, indexing="ij"), np.full(3, lo32, np.float32), np.full(3, h, np.float32)


def _ball(X, c, r):
    (x, y, z) = X
    return np.float32(r) - np.sqrt((x - np.float32(c[0])) ** 2 + (y - np.float32(c[1])) ** 2 + (z - np.float32(c[2])) ** 2)


def planted_field(n=48):
    """Five pieces on [-0.5, 0.5]^3 at level 0, the max of: a ball r = 0.3 minus a ball r = 0.12 at (0.05, 0, 0) (a body with a closed
    cavity), balls r = 0.06 at (0.4, 0.4, 0.4) and r = 0.05 at (-0.4, 0.38, -0.3) (floaters), and a ball r = 0.08 at (0.5, 0, 0), which the
    border of the grid cuts open.  Returns (field (n, n, n) float32, lo (3,), h (3,))."""
    X, lo, h = _lattice(n)
    body = np.minimum(_ball(X, (0, 0, 0), 0.3), -_ball(X, (0.05, 0, 0), 0.12))
    f = np.maximum.reduce([body, _ball(X, (0.4, 0.4, 0.4), 0.06), _ball(X, (-0.4, 0.38, -0.3), 0.05), _ball(X, (0.5, 0, 0), 0.08)])
    return f.astype(np.float32), lo, h


def ball_field(n=48, r=0.2):
    X, lo, h = _lattice(n)
    return _ball(X, (0, 0, 0), r).astype(np.float32), lo, h


def helix_field(n=96, turns=6.5, radius=0.3, margin=8):
    """A one-voxel-thick tube wound ``turns`` times around the z axis: +1 on a chain of grid points, each next to the one before along one
    axis, -1 elsewhere; level 0.  One long thin component: long parent chains for a union-find."""
    t = np.linspace(0.0, 2 * np.pi * turns, 40 * n * int(np.ceil(turns)))
    c = (n - 1) / 2.0
    path = np.stack([c + radius * (n - 1) * np.cos(t), c + radius * (n - 1) * np.sin(t), margin + (n - 1 - 2 * margin) * t / t[-1]], axis=1)
    pts = np.rint(path).astype(np.int64)
    pts = pts[np.concatenate([[True], (np.diff(pts, axis=0) != 0).any(axis=1)])]
    f = np.full((n, n, n), -1.0, np.float32)
    cur = pts[0].copy()
    f[tuple(cur)] = 1.0
    for p in pts[1:]:
        for a in range(3):                                   # one axis at a time: consecutive tube points share a grid edge
            while cur[a] != p[a]:
                cur[a] += 1 if p[a] > cur[a] else -1
                f[tuple(cur)] = 1.0
    _, lo, h = _lattice(n)
    return f, lo, h
