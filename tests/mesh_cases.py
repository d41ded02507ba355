"""Test helper (numpy only): small hard meshes for the component kernels of sup-nerf_amd/csrc/snr_mesh.hip -- graphs a marching-
tetrahedra mesh never is.  Every mesh has at most 4097 vertices, so a lock-free union-find, a pointer chase and a wave-level merge meet
their worst cases in milliseconds.

``SHAPES``: name -> (V, faces, the component count the construction implies).  ``corpus()``: every shape in four numberings --
"ascending" (the faces as listed), and "shuffled", "reversed", "random" (the vertices as built / reversed / renamed by a seeded
permutation through ``mesh_restatement.permuted``, the faces shuffled by a seeded permutation) -- with the coordinates of ``coords``.
``many_objects()``: B = 67 objects for one packed call.  ``extreme_box_case()``: coordinates and labels for the boxes alone."""
import functools

import numpy as np

import mesh_restatement as MR

NUMBERINGS = ("ascending", "shuffled", "reversed", "random")
FLT_MAX = np.finfo(np.float32).max
DENORM_MIN = np.float32(2.0 ** -149)


def coords(n, seed):
    """(n, 3) fp32: a seeded normal deviate times 2^k, k in [-8, 8] per coordinate (the idea of ``segment_sum_restatement.draw``): over
    16 binades almost every change of an operation order changes a rounded term."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 3)) * 2.0 ** rng.integers(-8, 9, (n, 3))).astype(np.float32)


def _f(rows):
    return np.asarray(rows, dtype=np.int32).reshape(-1, 3)


def _edges(i, j):
    """Faces (i, j, j): an edge as a degenerate triangle."""
    return np.stack([i, j, j], axis=1).astype(np.int32)


def fan(n, hub=0):
    """``n`` triangles (hub, r_k, r_k+1) around vertex ``hub``, the rim r_0..r_n the n + 1 indices after it: n + 2 vertices."""
    k = np.arange(n, dtype=np.int32)
    return np.stack([np.full(n, hub, np.int32), hub + 1 + k, hub + 2 + k], axis=1)


def _binary_tree(levels=12):
    """Faces (i, i + 2^k, i + 2^k) over 2^levels vertices, i the multiples of 2^(k+1), the largest k first: the last faces listed join
    neighbours, the first one joins the two halves -- every union but those of k = 0 meets trees already built if taken in reverse."""
    out = []
    for k in range(levels - 1, -1, -1):
        i = np.arange(0, 2 ** levels, 2 ** (k + 1), dtype=np.int32)
        out.append(_edges(i, i + 2 ** k))
    return np.concatenate(out)


def _repeated_indices():
    """Ordinary faces mixed with (i, i, i), (i, i, j), (i, j, i) and (i, j, j): {0..4} by two ordinary faces, {5} alone in (5, 5, 5),
    {6, 7} by (6, 6, 7) alone (only the pair (v0, v2) joins them), {8, 9} by (8, 9, 8), {10, 11} by (10, 11, 11), {12, 13, 14} by an
    ordinary face and (13, 13, 13), {15} no face names: 7 components over 16 vertices."""
    return _f([[0, 1, 2], [5, 5, 5], [6, 6, 7], [2, 3, 4], [8, 9, 8], [10, 11, 11], [12, 14, 13], [13, 13, 13], [4, 4, 0], [1, 3, 1]])


def _shapes():
    i = np.arange(4096, dtype=np.int32)
    leaves = 1 + i
    s = {}
    s["edge path"] = (4097, _edges(i, i + 1), 1)
    s["triangle strip"] = (4097, np.stack([i[:-1], i[:-1] + 1, i[:-1] + 2], axis=1), 1)
    s["star on vertex 0"] = (4097, _edges(np.zeros(4096, np.int32), leaves), 1)
    s["star on the last vertex"] = (4097, _edges(np.full(4096, 4096, np.int32), i), 1)
    s["two interleaved combs"] = (4097, _edges(i[:-1], i[:-1] + 2), 2)
    s["one face 1024 times"] = (5, np.tile(_f([[1, 3, 2]]), (1024, 1)), 3)                  # {1, 2, 3}, and 0 and 4 alone
    s["repeated indices"] = (16, _repeated_indices(), 7)
    s["64 singletons, a fan of 300"] = (64 + 302, fan(300, hub=64), 65)
    s["binary-tree merge order"] = (4096, _binary_tree(12), 1)
    return s


SHAPES = _shapes()


def numbered(n_verts, faces, numbering, seed):
    """(verts, faces) of a shape in one of ``NUMBERINGS``; the coordinates travel with their vertices."""
    rng = np.random.default_rng(seed)
    verts = coords(n_verts, seed + 1)
    if numbering == "ascending":
        return verts, np.ascontiguousarray(faces, np.int32)
    perm = {"shuffled": np.arange(n_verts), "reversed": np.arange(n_verts)[::-1].copy(), "random": rng.permutation(n_verts)}[numbering]
    v, f = MR.permuted(verts, faces, perm, rng.permutation(faces.shape[0]))
    return v, np.ascontiguousarray(f, np.int32)


@functools.lru_cache(maxsize=None)
def corpus():
    """[(tag, verts (V, 3) fp32, faces (F, 3) int32, the component count)], every shape in every numbering, drawn once."""
    out = []
    for s, (name, (n_verts, faces, n_comps)) in enumerate(SHAPES.items()):
        for k, numbering in enumerate(NUMBERINGS):
            v, f = numbered(n_verts, faces, numbering, 100 * s + 10 * k)
            out.append((f"{name}, {numbering}", v, f, n_comps))
    return out


# ---------------------------------------------------------------------------------------------------------------- many objects
_SMALL = {"points": (3, _f([]), 3), "triangle": (3, _f([[0, 1, 2]]), 1), "two triangles": (4, _f([[0, 1, 2], [1, 3, 2]]), 1),
          "tetrahedron": (4, _f([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]]), 1)}
MANY_EMPTY = (0, 1, 30, 31, 32, 65, 66)
MANY_FAN, MANY_PATH = 12, 47


@functools.lru_cache(maxsize=None)
def many_objects():
    """B = 67 objects for one packed call: [(kind, verts, faces, the component count)].

    Objects 0, 1 (a leading run), 30, 31, 32 (a run in the middle) and 65, 66 (a trailing run) are empty, V = F = 0.  Object 12 is a fan
    of 300 triangles (302 vertices), object 47 an edge path of 600 vertices (599 faces (i, i + 1, i + 1)).  The other 58 cycle through
    three lone points (V = 3, F = 0: an empty entry of the face offsets only), a triangle (V = 3), two triangles (V = 4) and a
    tetrahedron (V = 4), in that order from object 2 on.  So the fan's vertices are [34, 336), the path's [445, 1045), of sum V = 1104 (sum F = 998):
    both start and end strictly inside a wave of 64 and a block of 256, each of them crosses block borders (256; 512, 768, 1024), and
    the face offsets have runs of equal entries of their own wherever lone points stand beside an empty object."""
    kinds = list(_SMALL)
    out, k = [], 0
    for b in range(67):
        if b in MANY_EMPTY:
            out.append(("empty", np.zeros((0, 3), np.float32), _f([]), 0))
        elif b == MANY_FAN:
            out.append(("fan", coords(302, 7000 + b), fan(300), 1))
        elif b == MANY_PATH:
            i = np.arange(599, dtype=np.int32)
            out.append(("path", coords(600, 7000 + b), _edges(i, i + 1), 1))
        else:
            n_verts, faces, n_comps = _SMALL[kinds[k % 4]]
            out.append((kinds[k % 4], coords(n_verts, 7000 + b), faces.copy(), n_comps))
            k += 1
    return out


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def packed(objects):
    """(verts (sum V, 3), faces (sum F, 3) with local indices, vert_offset, face_offset) of [(verts, faces), ...]."""
    verts = np.concatenate([np.asarray(v, np.float32).reshape(-1, 3) for v, _ in objects] + [np.zeros((0, 3), np.float32)])
    faces = np.concatenate([np.asarray(f, np.int32).reshape(-1, 3) for _, f in objects] + [_f([])])
    return verts, faces, offsets([len(v) for v, _ in objects]), offsets([len(f) for _, f in objects])


def entry_of(off, i):
    """``mesh_entry_of`` of snr_packed_mesh.hpp for an array of items: the largest b < n with off[b] <= i -- empty entries are skipped."""
    return np.searchsorted(np.asarray(off)[:-1], np.asarray(i), side="right") - 1


# ---------------------------------------------------------------------------------------------------------------- the boxes alone
def extreme_box_case():
    """(verts (769, 3) fp32, labels (769,) int32, C = 6) for ``snr_mesh_boxes`` alone: finite coordinates where the order-preserving key
    of the box matters.  Components 0..3 take the vertices g mod 4 with values drawn from a pool of +-FLT_MAX / 4, +-1 and its
    neighbours one ulp away, +-0, denormals and ordinary numbers; +FLT_MAX stands at vertex 0 (the first lane of a wave), -FLT_MAX at
    vertex 63 (the last lane), both again at vertex 337 (a lane of another wave, another block) and -FLT_MAX at vertex 768 (the lone
    vertex of the partial last block).  Component 4 = the vertices {5, 70, 300}, which hold only -0.0 and +0.0 in x and y and only
    denormals in z.  Component 5 = the vertices {6, 200}: pairs one ulp apart (1 and its successor, -1 and its predecessor, the two
    smallest denormals)."""
    rng = np.random.default_rng(41)
    one_up, minus_one_down = np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(-1), np.float32(-2))
    pool = np.array([FLT_MAX / 4, -FLT_MAX / 4, 1.0, one_up, -1.0, minus_one_down, 0.0, -0.0, DENORM_MIN, -DENORM_MIN, 2.0 ** -127,
                     -2.0 ** -127, 3.5, -3.5, 2.0 ** -20, -2.0 ** -20], dtype=np.float32)
    n = 3 * 256 + 1
    verts = pool[rng.integers(0, pool.shape[0], (n, 3))]
    labels = (np.arange(n) % 4).astype(np.int32)
    verts[0, 0], verts[63, 1], verts[337], verts[768, 2] = FLT_MAX, -FLT_MAX, (FLT_MAX, -FLT_MAX, FLT_MAX), -FLT_MAX
    labels[[5, 70, 300]] = 4
    verts[5], verts[70], verts[300] = (-0.0, 0.0, DENORM_MIN), (0.0, -0.0, -DENORM_MIN), (-0.0, 0.0, 2 * DENORM_MIN)
    labels[[6, 200]] = 5
    verts[6], verts[200] = (1.0, -1.0, DENORM_MIN), (one_up, minus_one_down, 2 * DENORM_MIN)
    return verts, labels, 6
