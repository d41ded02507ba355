"""The mesh-component kernels of sup-nerf_amd/csrc/snr_mesh.hip, each alone through the C ABI, on the small hard meshes of
tests/mesh_cases.py: ``snr_mesh_hook`` (the lock-free union-find: chains, stars whose every thread meets in one word, interleaved
components, repeated faces and indices, a bad face that is skipped while the others are united), ``snr_mesh_flatten`` on hand-made
forests, ``snr_mesh_label``, ``snr_mesh_boxes`` on hand-made labels and extreme coordinates, ``snr_mesh_face_terms`` bit for bit
against ``mesh_restatement.face_terms_exact`` -- every one also on B = 67 objects in one packed call with runs of empty objects, which is
what ``mesh_entry_of`` (the offset search of all four packed-mesh families) has to get right; and the other three families on that
layout, the packed call against the per-object calls.

Every integer output is compared exactly, every float64 term bit for bit.  Every output buffer of every call lies between guard bands
(``segment_sum_restatement.banded``), checked after one synchronise at the end of each test."""
import numpy as np
import pytest
import torch

import mesh_cases as MC
import mesh_restatement as MR
from segment_sum_restatement import banded as _banded, bands_intact as _bands_intact, same_bits
from oracle_bands import amd, dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

I32, I64, U8, F32, F64 = torch.int32, torch.int64, torch.uint8, torch.float32, torch.float64
BAD_INDICES = ("V", "V + 12345", -1, 2 ** 31 - 1)
NAN = float("nan")


def _np(t):
    return t.detach().cpu().numpy()


class _Abi:
    """The library, the pointer and stream helpers of ``ops``, and the guard bands of every output buffer handed out by ``out``."""

    def __init__(self, amd, dev):  # noqa: F811
        self.lib, self.P, self.st, self.dev = amd._lib.lib(), amd.ops._ptr, amd.ops._stream(dev), dev
        self.checks = []

    def up(self, a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(self.dev)

    def out(self, n, dtype, fill):
        full, mid = _banded(int(n), dtype, self.dev, fill)
        self.checks.append((full, int(n), fill))
        return mid

    def bands_intact(self):
        torch.cuda.synchronize()
        for full, n, fill in self.checks:
            assert _bands_intact(full, n, fill), (n, fill, full.dtype)
        return len(self.checks)


class _Mesh:
    """A packed mesh on the host and on the device: [(verts, faces), ...] per object."""

    def __init__(self, k, objects):
        self.objects = objects
        self.verts, self.faces, self.voff, self.foff = MC.packed(objects)
        self.B, self.nV, self.nF = len(objects), int(self.voff[-1]), int(self.foff[-1])
        self.d_verts, self.d_faces = k.up(self.verts, F32), k.up(self.faces, I32)
        self.d_voff, self.d_foff = k.up(self.voff, I64), k.up(self.foff, I64)

    def per_object(self, packed_rows, off=None):
        off = self.voff if off is None else off
        return [packed_rows[off[b]:off[b + 1]] for b in range(self.B)]

    def low(self, faces=None):
        """(sum V,) the smallest local index every vertex reaches, object by object: what the roots must be."""
        faces = self.faces if faces is None else faces
        return np.concatenate([MR.reach_smallest(v.shape[0], f) for (v, _), f in zip(self.objects, self.per_object(faces, self.foff))] +
                              [np.zeros(0, np.int64)]).astype(np.int32)


def _hook(k, m, d_faces=None):
    """``snr_mesh_hook`` on mesh ``m`` (with other faces of the same counts if given): (parent (sum V,) int32, bad (1,) int32)."""
    parent, bad = k.out(m.nV, I32, -7), k.out(1, I32, -7)
    bad.zero_()
    faces = m.d_faces if d_faces is None else d_faces
    assert k.lib.snr_mesh_hook(k.P(faces, I32), k.P(m.d_voff, I64), k.P(m.d_foff, I64), m.B, m.nV, m.nF, k.P(parent, I32), k.P(bad, I32),
                               k.st) == 0
    return parent, bad


def _flatten(k, m, parent):
    root, is_root = k.out(m.nV, I32, -7), k.out(m.nV, U8, 255)
    assert k.lib.snr_mesh_flatten(k.P(parent, I32), k.P(m.d_voff, I64), m.B, m.nV, k.P(root, I32), k.P(is_root, U8), k.st) == 0
    return root, is_root


def _local_index(m):
    return (np.arange(m.nV) - m.voff[MC.entry_of(m.voff, np.arange(m.nV))]).astype(np.int32)


def _check_forest(m, parent, want_low, tag):
    """The contract of the hook's parent array: parent[v] <= v within the object, and following it from every vertex ends at the
    smallest vertex index the vertex reaches."""
    p, local = _np(parent), _local_index(m)
    assert p.dtype == np.int32 and (p >= 0).all() and (p <= local).all(), tag
    roots = np.concatenate([MR.roots_of(x) for x in m.per_object(p)] + [np.zeros(0, np.int32)])
    assert np.array_equal(roots, want_low), tag


@pytest.fixture(scope="module")
def corpus_low():
    """tag -> the smallest index every vertex of the corpus mesh reaches, computed once."""
    return {tag: MR.reach_smallest(v.shape[0], f).astype(np.int32) for tag, v, f, _ in MC.corpus()}


@pytest.fixture(scope="module")
def many():
    objs = [(v, f) for _, v, f, _ in MC.many_objects()]
    assert len(objs) == 67
    return objs


# ------------------------------------------------------------------ snr_mesh_hook
def test_hook_on_the_corpus(amd, dev, corpus_low, many):  # noqa: F811
    """Every corpus mesh and the B = 67 layout, twice: the forest contract, the flag 0, and the same FLATTENED roots from both runs (the
    parent array itself is the implementation's)."""
    k = _Abi(amd, dev)
    cases = [(tag, _Mesh(k, [(v, f)]), corpus_low[tag]) for tag, v, f, _ in MC.corpus()]
    m67 = _Mesh(k, many)
    cases.append(("B = 67", m67, m67.low()))
    for tag, m, low in cases:
        roots = []
        for _ in range(2):
            parent, bad = _hook(k, m)
            _check_forest(m, parent, low, tag)
            assert bad.tolist() == [0], tag
            root, is_root = _flatten(k, m, parent)
            roots.append(root)
            assert np.array_equal(_np(root), low) and np.array_equal(_np(is_root), (low == _local_index(m)).astype(np.uint8)), tag
        assert torch.equal(roots[0], roots[1]), tag
    assert k.bands_intact() == 4 * 2 * len(cases)


def _bad_value(name, V):
    return {"V": V, "V + 12345": V + 12345}.get(name, name)


def test_hook_skips_a_bad_face_and_unites_the_rest(amd, dev, many):  # noqa: F811
    """One face bad -- V, V + 12345, -1, 2^31 - 1 in each of the three slots: the flag is 1 and the forest is that of the other faces.
    On the edge path (random numbering) the missing face cuts the path in two; on the B = 67 layout the bad face sits in the path
    object, and an index that is the neighbouring object's but not its own is bad too."""
    k = _Abi(amd, dev)
    tag, v, f, _ = next(c for c in MC.corpus() if c[0] == "edge path, random")
    m = _Mesh(k, [(v, f)])
    m67 = _Mesh(k, many)
    runs = 0
    for mesh, b, row, V in ((m, 0, m.nF // 2, m.nV), (m67, MC.MANY_PATH, int(m67.foff[MC.MANY_PATH]) + 300, 600)):
        rest = mesh.faces.copy()
        rest[row] = 0                                                            # (a face of three equal, valid indices unites nothing)
        want = mesh.low(rest)
        assert len(np.unique(want[mesh.voff[b]:mesh.voff[b + 1]])) == 2 and len(np.unique(mesh.low()[mesh.voff[b]:mesh.voff[b + 1]])) == 1
        for slot in range(3):
            for name in BAD_INDICES:
                faces = mesh.faces.copy()
                faces[row, slot] = _bad_value(name, V)
                parent, bad = _hook(k, mesh, k.up(faces, I32))
                assert bad.tolist() == [1], (slot, name)
                _check_forest(mesh, parent, want, (slot, name))
                runs += 1
    # a triangle (V = 3) whose neighbour has four vertices: index 3 is the neighbour's alone
    kinds = [kind for kind, _, _, _ in MC.many_objects()]
    b = next(b for b in range(66) if kinds[b] == "triangle" and kinds[b + 1] == "two triangles")
    rest = m67.faces.copy()
    rest[m67.foff[b]] = 0
    want = m67.low(rest)
    assert want[m67.voff[b]:m67.voff[b + 1]].tolist() == [0, 1, 2]
    for slot in range(3):
        faces = m67.faces.copy()
        faces[m67.foff[b], slot] = 3
        parent, bad = _hook(k, m67, k.up(faces, I32))
        assert bad.tolist() == [1], slot
        _check_forest(m67, parent, want, ("the neighbour's index", slot))
        runs += 1
    assert k.bands_intact() == 2 * runs


# ------------------------------------------------------------------ snr_mesh_flatten
def test_flatten_on_hand_made_forests(amd, dev, many):  # noqa: F811
    """Any forest with parent[i] <= i: the identity, the chain parent[i] = i - 1 over 4097 vertices (one thread walks 4096 links), a
    star, a seeded random forest (parent[i] uniform in [0, i]), and the same per object of the B = 67 layout with local indices."""
    k = _Abi(amd, dev)
    rng = np.random.default_rng(23)
    n = 4097
    i = np.arange(n)
    star = np.zeros(n, np.int64)
    forests = {"identity": i, "chain": np.maximum(i - 1, 0), "star": star, "random forest": rng.integers(0, i + 1)}
    one = _Mesh(k, [(np.zeros((n, 3), np.float32), np.zeros((0, 3), np.int32))])
    m67 = _Mesh(k, many)
    cases = [(name, one, p) for name, p in forests.items()]
    sizes = np.diff(m67.voff)
    for name, make in (("B = 67 random", lambda s: rng.integers(0, np.arange(s) + 1)), ("B = 67 chains", lambda s: np.maximum(np.arange(s) - 1, 0)),
                       ("B = 67 identity", np.arange)):
        cases.append((name, m67, np.concatenate([make(int(s)) for s in sizes if s])))
    for name, m, parent in cases:
        assert parent.shape == (m.nV,) and (parent >= 0).all() and (parent <= _local_index(m)).all()
        want = np.concatenate([MR.roots_of(x) for x in m.per_object(parent)] + [np.zeros(0, np.int32)])
        root, is_root = _flatten(k, m, k.up(parent, I32))
        assert np.array_equal(_np(root), want), name
        assert np.array_equal(_np(is_root), (want == _local_index(m)).astype(np.uint8)), name
    assert not MR.roots_of(forests["chain"]).any() and 1 <= len(np.unique(MR.roots_of(forests["random forest"]))) < 64
    assert k.bands_intact() == 2 * len(cases)


# ------------------------------------------------------------------ snr_mesh_label
def _restated_roots(m, faces=None):
    """(root, root_scan) (sum V,) int32 as the pipeline would hand them to ``snr_mesh_label``, from the restatement."""
    low = m.low(faces)
    is_root = low == _local_index(m)
    scan = np.concatenate([np.cumsum(x) for x in m.per_object(is_root)] + [np.zeros(0, np.int64)]).astype(np.int32)
    return low, scan


def test_label_from_restated_roots(amd, dev, many):  # noqa: F811
    """vert_label and face_label of corpus meshes and of the B = 67 layout; then bad indices: a bad FIRST index gives face_label -1, a
    bad second or third beside a good first gives the label of the first (rule 2 reads nothing else)."""
    k = _Abi(amd, dev)
    tags = ("repeated indices, random", "64 singletons, a fan of 300, reversed", "two interleaved combs, random", "one face 1024 times, shuffled")
    cases = [(c[0], _Mesh(k, [(c[1], c[2])])) for c in MC.corpus() if c[0] in tags]
    assert len(cases) == len(tags)
    cases.append(("B = 67", _Mesh(k, many)))
    calls = 0
    for tag, m in cases:
        root, scan = _restated_roots(m)
        rng = np.random.default_rng(m.nF)
        faces = m.faces.copy()
        spoiled = [faces]
        for name in BAD_INDICES:
            f2 = m.faces.copy()
            rows = rng.choice(m.nF, size=min(m.nF, 9), replace=False)
            for j, row in enumerate(rows):
                b = int(MC.entry_of(m.foff, row))
                f2[row, j % 3] = _bad_value(name, int(m.voff[b + 1] - m.voff[b]))
            spoiled.append(f2)
        for f2 in spoiled:
            want = [MR.labels_from(r, s, f, r.shape[0]) for r, s, f in zip(m.per_object(root), m.per_object(scan), m.per_object(f2, m.foff))]
            vert_label, face_label = k.out(m.nV, I32, -7), k.out(m.nF, I32, -7)
            assert k.lib.snr_mesh_label(k.P(k.up(root, I32), I32), k.P(k.up(scan, I32), I32), k.P(k.up(f2, I32), I32), k.P(m.d_voff, I64),
                                        k.P(m.d_foff, I64), m.B, m.nV, m.nF, k.P(vert_label, I32), k.P(face_label, I32), k.st) == 0
            calls += 1
            want_f = np.concatenate([w[1] for w in want])
            assert np.array_equal(_np(vert_label), np.concatenate([w[0] for w in want])), tag
            assert np.array_equal(_np(face_label), want_f), tag
            if f2 is not faces:
                assert (want_f == -1).sum() >= 1 and (want_f[(f2 != m.faces).any(1)] >= 0).any(), tag      # both kinds of bad face took part
    assert k.bands_intact() == 2 * calls


# ------------------------------------------------------------------ snr_mesh_boxes
def _boxes(k, verts, labels, voff, coff, tag):
    """``snr_mesh_boxes`` against ``boxes_from`` object by object; a component no vertex counts for: its count of 0 alone."""
    B, nV, nC = len(voff) - 1, int(voff[-1]), int(coff[-1])
    n, lo, hi = k.out(nC, I64, -1), k.out(nC * 3, F32, NAN), k.out(nC * 3, F32, NAN)
    assert k.lib.snr_mesh_boxes(k.P(k.up(verts, F32)), k.P(k.up(labels, I32), I32), k.P(k.up(voff, I64), I64), k.P(k.up(coff, I64), I64), B,
                                nV, nC, k.P(n, I64), k.P(lo), k.P(hi), k.st) == 0
    want = [MR.boxes_from(verts[voff[b]:voff[b + 1]], labels[voff[b]:voff[b + 1]], int(coff[b + 1] - coff[b])) for b in range(B)]
    want_n = np.concatenate([w[0] for w in want])
    assert np.array_equal(_np(n), want_n), tag
    seen = want_n > 0
    for got, w in ((lo, np.concatenate([w[1] for w in want])), (hi, np.concatenate([w[2] for w in want]))):
        assert np.array_equal(_np(got).reshape(nC, 3)[seen], w[seen]), tag       # (== on values: -0 and +0 count as equal)
    return want_n


def test_boxes_on_hand_made_labels(amd, dev, many):  # noqa: F811
    """Label patterns that stress the merge of ``mesh_box_kernel`` -- 64 groups in every wave, two, one; the same first group in waves 0
    and 2 of a block but not in 1 and 3; a partial last block (nV = 3 * 256 + 1); labels that are not the object's (-1, C, 2^31 - 1,
    another object's id) at lane 0 of a wave and over a whole wave; the extreme coordinates; B = 67 with ``comp_offset``."""
    k = _Abi(amd, dev)
    n = 3 * 256 + 1
    g = np.arange(n)
    verts = MC.coords(n, 5)
    one = np.array([0, n], np.int64)
    for tag, labels, C in (("g mod 64", g % 64, 64), ("g mod 2", g % 2, 2), ("all equal", np.zeros(n, np.int64), 1),
                           ("all equal, the middle one of three", np.ones(n, np.int64), 3)):
        counts = _boxes(k, verts, labels, one, np.array([0, C]), tag)
        assert counts.sum() == n
    # the first group (lane 0's) of waves 0 and 2 of every block is component 7, of waves 1 and 3 another one
    lane, wave = g % 64, (g // 64) % 4
    labels = 1 + lane % 3
    labels[lane == 0] = np.where(wave[lane == 0] % 2 == 0, 7, 5 + wave[lane == 0] // 2)
    labels[(lane == 9) & (wave == 1)] = 7                                        # (and in wave 1 the component is a later group)
    counts = _boxes(k, verts, labels, one, np.array([0, 8]), "first groups")
    assert counts[7] == 7 + 3 and counts[0] == 0 and counts[4] == 0 and counts[5] == 3 and counts[6] == 3 and counts.sum() == n
    # labels that are not the object's: two objects of 3 and 5 components, 448 and 321 vertices
    voff, coff = np.array([0, 448, n]), np.array([0, 3, 8])
    base = np.where(g < 448, g % 3, g % 5)
    for name, value in (("-1", -1), ("C_b", None), ("2^31 - 1", 2 ** 31 - 1), ("another object's id", 4), ("below the object's ids", -2)):
        labels = base.copy()
        alien = np.zeros(n, bool)
        alien[[0, 64, 192, 256, 448, 512, 768]] = True                           # lane 0 of a wave (448 = 7 * 64)
        alien[128:192] = True                                                    # a whole wave of object 0
        alien[576:640] = True                                                    # and one of object 1
        alien[[5, 70, 450]] = True
        labels[alien] = np.where(g[alien] < 448, 3, 5) if value is None else value
        if name == "another object's id":
            labels[alien & (g >= 448)] = -3 + 1                                  # for object 1, an id of object 0: comp_offset + label = 1
        counts = _boxes(k, verts, labels, voff, coff, name)
        assert counts.sum() == n - alien.sum(), name
    verts_x, labels_x, C = MC.extreme_box_case()
    counts = _boxes(k, verts_x, labels_x, one, np.array([0, C]), "extreme coordinates")
    assert counts.tolist()[4:] == [3, 2]
    assert _boxes(k, verts_x[::-1].copy(), labels_x[::-1].copy(), one, np.array([0, C]), "extreme coordinates, reversed").sum() == n
    # B = 67: the true labels, per-object component offsets with their own runs of empties
    m = _Mesh(k, many)
    root, scan = _restated_roots(m)
    vert_label = np.concatenate([MR.labels_from(r, s, np.zeros((0, 3)), r.shape[0])[0] for r, s in zip(m.per_object(root), m.per_object(scan))])
    coff = MC.offsets([c for _, _, _, c in MC.many_objects()])
    counts = _boxes(k, m.verts, vert_label, m.voff, coff, "B = 67")
    assert counts.sum() == m.nV and coff[-1] == counts.shape[0] and (counts > 0).all()
    assert k.bands_intact() == 3 * (4 + 1 + 5 + 2 + 1)


# ------------------------------------------------------------------ snr_mesh_face_terms
def _face_terms(k, m, d_faces, root, order):
    area, vol = k.out(m.nF, F64, NAN), k.out(m.nF, F64, NAN)
    d_order = None if order is None else k.up(order, I64)
    assert k.lib.snr_mesh_face_terms(k.P(m.d_verts), k.P(d_faces, I32), k.P(k.up(root, I32), I32), k.P(d_order, I64), k.P(m.d_voff, I64),
                                     k.P(m.d_foff, I64), m.B, m.nV, m.nF, k.P(area, F64), k.P(vol, F64), k.st) == 0
    return _np(area), _np(vol)


def _exact_terms(m, faces, root):
    """``face_terms_exact`` object by object with p0 = the vertex root[v0]; 0, 0 for a face with an index outside its object."""
    area, vol = np.zeros(m.nF), np.zeros(m.nF)
    for b, ((v, _), f, r) in enumerate(zip(m.objects, m.per_object(faces, m.foff), m.per_object(root))):
        ok = ((f >= 0) & (f < v.shape[0])).all(1)
        a, w = MR.face_terms_exact(v, f[ok], v.astype(np.float64)[r[f[ok][:, 0]]])
        sl = np.arange(m.foff[b], m.foff[b + 1])[ok]
        area[sl], vol[sl] = a, w
    return area, vol


def test_face_terms_bit_for_bit(amd, dev, many):  # noqa: F811
    """Both float64 terms of every face equal ``face_terms_exact`` in every bit -- the products, differences and sums in the kernel's
    order, one IEEE square root -- with ``order`` NULL, the identity and a seeded permutation; a face with a bad index and an ``order``
    entry outside [0, sum F) (-1, sum F) give 0, 0; a degenerate face has area exactly 0.

    On the MI355X the device's float64 square root gave numpy's bits on every term of every case here (0 of them differ)."""
    k = _Abi(amd, dev)
    tags = ("triangle strip, ascending", "triangle strip, random", "64 singletons, a fan of 300, reversed", "repeated indices, random",
            "edge path, shuffled", "one face 1024 times, random")
    cases = [(c[0], _Mesh(k, [(c[1], c[2])])) for c in MC.corpus() if c[0] in tags]
    assert len(cases) == len(tags)
    cases.append(("B = 67", _Mesh(k, many)))
    calls, terms, off_by = 0, 0, 0
    for tag, m in cases:
        root = m.low()
        rng = np.random.default_rng(m.nV)
        faces = m.faces.copy()
        for j, row in enumerate(rng.choice(m.nF, size=min(m.nF // 2, 8), replace=False)):           # some faces with a bad index
            b = int(MC.entry_of(m.foff, row))
            faces[row, j % 3] = _bad_value(BAD_INDICES[j % 4], int(m.voff[b + 1] - m.voff[b]))
        for f2 in (m.faces, faces):
            want_a, want_v = _exact_terms(m, f2, root)
            perm = rng.permutation(m.nF)
            holes = perm.copy()
            holes[rng.choice(m.nF, size=min(m.nF, 4), replace=False)] = (-1, m.nF, -2 ** 40, 2 ** 40)[:min(m.nF, 4)]
            for order in (None, np.arange(m.nF), perm, holes):
                got_a, got_v = _face_terms(k, m, k.up(f2, I32), root, order)
                calls += 1
                idx = np.arange(m.nF) if order is None else order
                inside = (idx >= 0) & (idx < m.nF)
                wa, wv = np.where(inside, want_a[np.where(inside, idx, 0)], 0.0), np.where(inside, want_v[np.where(inside, idx, 0)], 0.0)
                assert same_bits(got_v, wv).all(), (tag, "volume")
                off_by += int((~same_bits(got_a, wa)).sum())
                terms += m.nF
                assert same_bits(got_a, wa).all(), (tag, "area", int((~same_bits(got_a, wa)).sum()))
                assert not got_a[~inside].any() and not got_v[~inside].any()
                degenerate = (f2[:, 0] == f2[:, 1]) | (f2[:, 1] == f2[:, 2]) | (f2[:, 0] == f2[:, 2])
                assert not got_a[inside][degenerate[idx[inside]]].any(), tag
        assert (want_a != 0).any() or tag.startswith("edge path"), tag
    print(f"face terms: {terms} area terms compared, {off_by} differ from numpy's square root in bits")
    assert k.bands_intact() == 2 * calls


# ------------------------------------------------------------------ the other three families on B = 67
def _to_gpu(objects, dev):  # noqa: F811
    return [(torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev), torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(dev))
            for v, f in objects]


def _same(x, y):
    if torch.is_tensor(x):
        return torch.is_tensor(y) and x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y)
    return x == y


def test_smoothing_on_many_objects(amd, dev, many):  # noqa: F811
    """``mesh_adjacency`` and ``smooth_mesh`` of B = 67 in one packed call equal the 67 per-object calls (which
    tests/test_mesh_smooth_gpu.py holds to the restatement), the empty objects included."""
    from supnerf_amd import geometry as G
    meshes = _to_gpu(many, dev)
    adjs = G.mesh_adjacency(meshes)
    assert len(adjs) == 67
    for b, (mesh, a) in enumerate(zip(meshes, adjs)):
        one = G.mesh_adjacency(mesh)
        for name, x, y in zip(G.Adjacency._fields, a, one):
            assert _same(x, y), (b, name)
    assert int(adjs[MC.MANY_FAN].degree[0]) == 301 and adjs[MC.MANY_PATH].nbr.shape[0] == 2 * 599 and adjs[0].nbr_start.tolist() == [0]
    for pin in (None, "boundary"):
        packed = G.smooth_mesh(meshes, 3, pin=pin, adjacency=adjs if pin else None)
        for b, mesh in enumerate(meshes):
            assert _same(packed[b].verts, G.smooth_mesh(mesh, 3, pin=pin).verts), (b, pin)
    assert not torch.equal(G.smooth_mesh(meshes, 3, pin=None)[MC.MANY_PATH].verts, meshes[MC.MANY_PATH][0])


def test_simplification_on_many_objects(amd, dev, many):  # noqa: F811
    """``simplify_mesh`` of B = 67 in one packed call, one cell edge per object, equals the 67 per-object calls, the empty objects
    included."""
    from supnerf_amd import geometry as G
    meshes = _to_gpu(many, dev)
    cells = [float(2.0 ** (b % 5 - 1) * 1.5) for b in range(67)]
    for placement in ("quadric", "mean"):
        packed = G.simplify_mesh(meshes, cells, placement=placement, drop_unreferenced=False)
        assert len(packed) == 67
        for b, mesh in enumerate(meshes):
            one = G.simplify_mesh(mesh, cells[b], placement=placement, drop_unreferenced=False)
            for name, x, y in zip(G.Simplified._fields, packed[b], one):
                assert (x is None and y is None) or _same(x, y), (b, name, placement)
        assert 1 <= packed[MC.MANY_FAN].verts.shape[0] <= 302 and packed[0].verts.shape == (0, 3)
        assert sum(int(s.faces.shape[0]) for s in packed) > 0


def test_rasteriser_on_many_objects(amd, dev, many):  # noqa: F811
    """``rasterize(..., per_object=True)`` of B = 67 at 8 x 8 per image equals the 67 single calls: the faces as indices into the
    object's own list, depth and weights bit for bit; an empty object gives an empty image."""
    from supnerf_amd import geometry as G
    meshes = _to_gpu(many, dev)
    mats = np.zeros((67, 3, 4), np.float32)
    for b, (v, _) in enumerate(many):                                            # each object scaled to 0.9 across, two units ahead
        scale = np.float32(0.9 / float(np.abs(v).max())) if v.size else np.float32(1.0)
        mats[b, :, :3] = np.eye(3, dtype=np.float32) * scale
        mats[b, :, 3] = (0.1 * (b % 4) - 0.15, 0.05, 2.0)
    cam, size = (8.0, 8.0, 3.5, 3.5), (8, 8)
    r = G.rasterize(meshes, torch.from_numpy(mats).to(dev), cam, size, per_object=True)
    assert r.face.shape == (67, 8, 8)
    foff = MC.offsets([f.shape[0] for _, f in many])
    for b, mesh in enumerate(meshes):
        one = G.rasterize(mesh, torch.from_numpy(mats[b]).to(dev), cam, size, per_object=True)
        seen = one.face[0] >= 0
        assert torch.equal(r.face[b] >= 0, seen), b
        assert torch.equal(torch.where(seen, r.face[b] - int(foff[b]), r.face[b]), one.face[0]), b
        assert torch.equal(r.obj[b], torch.where(seen, torch.full_like(r.obj[b], b), r.obj[b])) and bool((r.obj[b][~seen] == -1).all()), b
        assert _same(r.depth[b], one.depth[0]) and _same(r.weights[b], one.weights[0]), b
        if many[b][1].shape[0] == 0:
            assert not bool(seen.any()), b
    hit = (r.face >= 0).flatten(1).any(1)
    print(f"rasteriser, B = 67: {int(hit.sum())} images see a face, {int((r.face >= 0).sum())} pixels in all")
    assert bool(hit[MC.MANY_FAN]) and int(hit.sum()) >= 10
