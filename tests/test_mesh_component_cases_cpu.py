"""The corpus of tests/mesh_cases.py on the host: every mesh has the components its construction implies and the labels scipy gives;
the fixed-order restatement lies within ``sum_bounds`` of the plain one; the step functions agree with the whole; and the corpus can tell
plausible wrong kernels from the right one -- each fault restated in numpy differs from the truth on at least one mesh."""
import numpy as np
import pytest

import mesh_cases as MC
import mesh_restatement as MR
import segment_sum_restatement as SS


def _scipy_labels(n_verts, faces):
    from test_mesh_components_cpu import _scipy_labels as labels
    return labels(n_verts, faces)


@pytest.fixture(scope="module")
def truth():
    """tag -> ``MR.components`` of every corpus mesh, computed once."""
    return {tag: MR.components(v, f) for tag, v, f, _ in MC.corpus()}


def test_the_corpus_has_the_components_its_construction_implies(truth):
    assert len(MC.corpus()) == 9 * 4 and max(v.shape[0] for _, v, _, _ in MC.corpus()) == 4097
    for tag, v, f, n_comps in MC.corpus():
        c = truth[tag]
        assert v.dtype == np.float32 and f.dtype == np.int32 and np.isfinite(v).all(), tag
        assert c["n_verts"].shape[0] == n_comps, (tag, c["n_verts"].shape[0], n_comps)
        n, want = _scipy_labels(v.shape[0], f)
        assert n == n_comps and np.array_equal(c["vert_label"], want) and np.array_equal(c["face_label"], want[f[:, 0]]), tag
    by_tag = {tag: truth[tag] for tag in truth}
    assert sorted(by_tag["two interleaved combs, ascending"]["n_verts"].tolist()) == [2048, 2049]
    assert by_tag["64 singletons, a fan of 300, ascending"]["n_verts"].tolist() == [1] * 64 + [302]
    assert by_tag["one face 1024 times, ascending"]["n_faces"].tolist() == [0, 1024, 0]
    assert by_tag["repeated indices, ascending"]["n_verts"].tolist() == [5, 1, 2, 2, 2, 3, 1]
    # "ascending" keeps the listed order: the binary tree starts with the face that joins the two halves
    assert SHAPE("binary-tree merge order")[1][0].tolist() == [0, 2048, 2048] and SHAPE("binary-tree merge order")[1].shape[0] == 4095


def SHAPE(name):
    return MC.SHAPES[name]


def test_the_many_object_layout():
    objs = MC.many_objects()
    assert len(objs) == 67
    kinds = [k for k, _, _, _ in objs]
    assert [b for b, k in enumerate(kinds) if k == "empty"] == list(MC.MANY_EMPTY) == [0, 1, 30, 31, 32, 65, 66]
    assert kinds[MC.MANY_FAN] == "fan" and kinds[MC.MANY_PATH] == "path" and {"points", "triangle", "two triangles", "tetrahedron"} <= set(kinds)
    _, _, voff, foff = MC.packed([(v, f) for _, v, f, _ in objs])
    assert (voff[-1], foff[-1]) == (1104, 998)
    assert (voff[MC.MANY_FAN], voff[MC.MANY_FAN + 1]) == (34, 336) and (voff[MC.MANY_PATH], voff[MC.MANY_PATH + 1]) == (445, 1045)
    for b in (MC.MANY_FAN, MC.MANY_PATH):                                        # borders strictly inside waves and blocks
        assert voff[b] % 64 and voff[b + 1] % 64 and foff[b] % 64 and foff[b + 1] % 64
    assert voff[-1] // 256 == 4                                                  # sum V crosses 256 four times, the last block is partial
    for tag, v, f, n_comps in objs:
        c = MR.components(v, f)
        assert c["n_verts"].shape[0] == n_comps, tag
        if v.shape[0]:
            assert _scipy_labels(v.shape[0], f)[0] == n_comps
    # the search: every item in its own object, empties skipped
    for off in (voff, foff):
        b = MC.entry_of(off, np.arange(off[-1]))
        assert (off[b] <= np.arange(off[-1])).all() and (np.arange(off[-1]) < off[b + 1]).all()


def test_the_step_functions_agree_with_the_whole(truth):
    for tag, v, f, _ in MC.corpus():
        c, V = truth[tag], v.shape[0]
        low = MR.reach_smallest(V, f)
        assert np.array_equal(MR.roots_of(low), low), tag                        # a flat forest is its own answer
        is_root = low == np.arange(V)
        vl, fl = MR.labels_from(low, np.cumsum(is_root), f, V)
        assert np.array_equal(vl, c["vert_label"]) and np.array_equal(fl, c["face_label"]) and vl.dtype == np.int32, tag
        n, lo, hi = MR.boxes_from(v, c["vert_label"], c["n_verts"].shape[0])
        assert np.array_equal(n, c["n_verts"]) and np.array_equal(lo, c["bbox_lo"]) and np.array_equal(hi, c["bbox_hi"]), tag
    chain = np.maximum(np.arange(4097) - 1, 0)
    assert not MR.roots_of(chain).any() and MR.roots_of(np.arange(5)).tolist() == [0, 1, 2, 3, 4]
    forest = np.array([0, 0, 1, 3, 3, 2])
    assert MR.roots_of(forest).tolist() == [0, 0, 0, 3, 3, 0]
    bad = np.array([[7, 0, 1], [0, 7, 1], [-1, 0, 0], [2, -5, 99]], np.int32)
    assert MR.labels_from(np.zeros(3), np.array([1, 1, 1]), bad, 3)[1].tolist() == [-1, 0, -1, 0]
    n, lo, hi = MR.boxes_from(np.arange(12, dtype=np.float32).reshape(4, 3), np.array([1, -1, 2, 2 ** 31 - 1]), 2)
    assert n.tolist() == [0, 1] and lo[1].tolist() == [0, 1, 2] and np.isinf(lo[0]).all()


def test_fixed_order_lies_within_the_any_order_bound(truth):
    """The reference alone satisfies the bound the GPU test keeps asserting: on the corpus, the B = 67 layout and the planted grid."""
    import iso_restatement as IR
    field, lo, h = MR.planted_field(48)
    cases = [(tag, v, f, truth[tag]) for tag, v, f, _ in MC.corpus()] + [(k, v, f, None) for k, v, f, _ in MC.many_objects()]
    cases.append(("planted",) + tuple(IR.extract(field, 0.0, lo, h)) + (None,))
    differ = 0
    for tag, v, f, c in cases:
        c = MR.components(v, f) if c is None else c
        fixed = MR.components_fixed_order(v, f, comp=c)
        ba, bv = MR.sum_bounds(c)
        assert fixed["area"].shape == c["area"].shape and fixed["volume"].dtype == np.float64, tag
        assert np.abs(fixed["area"] - c["area"]).max(initial=0.0) <= ba and np.abs(fixed["volume"] - c["volume"]).max(initial=0.0) <= bv, tag
        for name in ("vert_label", "face_label", "n_verts", "n_faces", "bbox_lo", "bbox_hi"):
            assert fixed[name] is c[name]
        differ += int((~SS.same_bits(fixed["area"], c["area"])).sum() + (~SS.same_bits(fixed["volume"], c["volume"])).sum())
    assert differ > 0                                                            # and it is another number: the order shows in the bits
    again = MR.components_fixed_order(*cases[-1][1:3])
    assert SS.same_bits(again["area"], MR.components_fixed_order(*cases[-1][1:3])["area"]).all()


# ------------------------------------------------------------------ the corpus can tell wrong kernels apart
def _caught(fault, true):
    """The corpus meshes on which ``fault(tag, verts, faces)`` differs from ``true(tag, verts, faces)`` (tuples of arrays)."""
    hits = []
    for tag, v, f, _ in MC.corpus():
        if not all(np.array_equal(a, b) for a, b in zip(fault(tag, v, f), true(tag, v, f))):
            hits.append(tag)
    return hits


def test_fault_uniting_only_the_first_pair_is_caught(truth):
    """(i): (v0, v1) united, (v0, v2) dropped."""
    hits = _caught(lambda tag, v, f: (MR.labels(v.shape[0], np.stack([f[:, 0], f[:, 1], f[:, 1]], 1))[0],), lambda tag, v, f: (truth[tag]["vert_label"],))
    assert any(t.startswith("repeated indices") for t in hits) and any(t.startswith("one face 1024 times") for t in hits)
    assert not any(t.startswith("edge path") for t in hits)                      # (faces (i, j, j): the first pair is the whole face)


def _labels_by_first_appearance(n_verts, faces):
    low = MR.reach_smallest(n_verts, faces)
    order = np.concatenate([faces.reshape(-1).astype(np.int64), np.arange(n_verts)])        # faces first, then whoever no face names
    seen, first_pos = np.unique(low[order], return_index=True)
    rank = np.empty(seen.shape[0], np.int64)
    rank[np.argsort(first_pos, kind="stable")] = np.arange(seen.shape[0])
    return rank[np.searchsorted(seen, low)].astype(np.int32)


def test_fault_numbering_by_first_appearance_is_caught(truth):
    """(ii): components numbered as the face list meets them, not by their smallest vertex index."""
    hits = _caught(lambda tag, v, f: (_labels_by_first_appearance(v.shape[0], f),), lambda tag, v, f: (truth[tag]["vert_label"],))
    assert "64 singletons, a fan of 300, ascending" in hits and any(t.startswith("repeated indices") for t in hits), hits
    # (the fault restated is a numbering of the same partition, and is right where the rule and the list agree)
    assert "edge path, ascending" not in hits


def _boxes_by_raw_bits(verts, labels, n_comps):
    """(iii): min / max over the raw fp32 bit patterns compared as unsigned integers."""
    bits = np.ascontiguousarray(verts, np.float32).view(np.uint32)
    lo, hi = np.full((n_comps, 3), 0xffffffff, np.uint32), np.zeros((n_comps, 3), np.uint32)
    for k in range(3):
        np.minimum.at(lo[:, k], labels, bits[:, k])
        np.maximum.at(hi[:, k], labels, bits[:, k])
    return lo.view(np.float32), hi.view(np.float32)


def test_fault_comparing_raw_bits_in_the_box_is_caught(truth):
    hits = _caught(lambda tag, v, f: _boxes_by_raw_bits(v, truth[tag]["vert_label"], truth[tag]["n_verts"].shape[0]),
                   lambda tag, v, f: (truth[tag]["bbox_lo"], truth[tag]["bbox_hi"]))
    assert len(hits) == len(MC.corpus())                                         # every mesh has a negative coordinate
    verts, labels, C = MC.extreme_box_case()
    n, lo, hi = MR.boxes_from(verts, labels, C)
    flo, fhi = _boxes_by_raw_bits(verts, labels, C)
    assert (n > 0).all() and np.isfinite(verts).all()
    assert not np.array_equal(flo, lo) and not np.array_equal(fhi, hi)
    # what the case holds: the extremes, a component of zeros of both signs, pairs one ulp apart
    assert hi[0, 0] == MC.FLT_MAX and lo[3, 1] == -MC.FLT_MAX and lo[1, 1] == -MC.FLT_MAX and hi[1, 2] == MC.FLT_MAX and lo[0, 2] == -MC.FLT_MAX
    assert (lo[4, :2] == 0).all() and (hi[4, :2] == 0).all() and lo[4, 2] == -MC.DENORM_MIN and hi[4, 2] == 2 * MC.DENORM_MIN
    assert lo[5].tolist() == [1.0, float(np.nextafter(np.float32(-1), np.float32(-2))), float(MC.DENORM_MIN)]
    assert hi[5].tolist() == [float(np.nextafter(np.float32(1), np.float32(2))), -1.0, float(2 * MC.DENORM_MIN)]
    signs = np.signbit(verts[labels == 4][:, :2])
    assert signs.any(0).all() and (~signs).any(0).all()                          # -0.0 and +0.0 both, in x and in y


def _entry_not_skipping(off, i):
    """(iv): a search that lands on the FIRST entry that starts at item i -- right while no entry is empty."""
    off, i = np.asarray(off), np.asarray(i)
    b = np.searchsorted(off, i, side="left")
    return np.where(off[np.minimum(b, off.shape[0] - 1)] == i, b, b - 1)


def test_fault_in_the_offset_search_is_caught():
    objs = [(v, f) for _, v, f, _ in MC.many_objects()]
    _, _, voff, foff = MC.packed(objs)
    full = [(v, f) for v, f in objs if f.shape[0]]
    _, _, voff_full, foff_full = MC.packed(full)
    for off in (voff_full, foff_full):                                           # no empty entry: the fault does not show
        items = np.arange(off[-1])
        assert np.array_equal(_entry_not_skipping(off, items), MC.entry_of(off, items))
    for off in (voff, foff):                                                     # B = 67: it does, and so does the plain "left" search
        items = np.arange(off[-1])
        want = MC.entry_of(off, items)
        assert not np.array_equal(_entry_not_skipping(off, items), want)
        assert not np.array_equal(np.searchsorted(off, items, "left"), want)
        # and what hangs on it: the empty entry starts where the right one does but holds nothing, so every index would be out of range
        b = _entry_not_skipping(off, items)
        assert np.array_equal(off[b], off[want]) and (off[b + 1] - off[b] == 0).any() and (off[want + 1] - off[want] > 0).all()
    assert MC.entry_of(voff, 0) == 2 and MC.entry_of(foff, 0) == 3               # the leading run (and the lone points) skipped


def _terms(tag, v, f, truth, formula):
    c = truth[tag]
    p0 = v.astype(np.float64)[c["first"][c["face_label"]]]
    return formula(v, f, p0)


def _volume_other_association(v, f, p0):
    x = np.asarray(v, np.float32).astype(np.float64)
    a, b, c = x[f[:, 0]] - p0, x[f[:, 1]] - p0, x[f[:, 2]] - p0
    ux, uy, uz = b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1], b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2], b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0]
    return (a[:, 0] * ux + (a[:, 1] * uy + a[:, 2] * uz)) / 6.0


def _area_other_order(v, f, p0):
    x = np.asarray(v, np.float32).astype(np.float64)
    a, b, c = x[f[:, 0]], x[f[:, 1]], x[f[:, 2]]
    e1, e2 = b - a, c - a
    nx, ny, nz = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return np.sqrt(nx * nx + (ny * ny + nz * nz)) / 2.0


def test_fault_in_the_order_of_a_term_or_of_the_sort_is_caught(truth):
    """(v): a re-associated last sum of the volume term, the squares of the area term added in another order, numpy's own term order
    (``MR.face_terms``), and a sort of the faces by component that is not stable (reversed within equal keys): each differs IN BITS from
    the fixed order on a corpus mesh."""
    faults = {"volume association": lambda v, f, p0: _volume_other_association(v, f, p0),
              "area order": lambda v, f, p0: _area_other_order(v, f, p0),
              "numpy volume": lambda v, f, p0: MR.face_terms(v, f, p0)[1]}
    exact = {"volume association": 1, "area order": 0, "numpy volume": 1}
    for name, formula in faults.items():
        hits, changed = [], 0
        for tag, v, f, _ in MC.corpus():
            same = SS.same_bits(_terms(tag, v, f, truth, formula), _terms(tag, v, f, truth, MR.face_terms_exact)[exact[name]])
            changed += int((~same).sum())
            if not same.all():
                hits.append(tag)
        print(f"{name}: {changed} terms differ in bits, on {len(hits)} meshes")
        assert any(t.startswith("triangle strip") for t in hits) and any(t.startswith("64 singletons, a fan") for t in hits), (name, hits)
    hits = []
    for tag, v, f, _ in MC.corpus():
        c = truth[tag]
        fixed = MR.components_fixed_order(v, f, comp=c)
        p0 = v.astype(np.float64)[c["first"][c["face_label"]]]
        terms = np.stack(MR.face_terms_exact(v, f, p0), axis=1)
        order, start, _ = SS.segments(c["face_label"], c["n_verts"].shape[0])
        unstable = np.concatenate([order[start[k]:start[k + 1]][::-1] for k in range(len(start) - 1)] + [order[:0]])
        assert np.array_equal(c["face_label"][unstable], c["face_label"][order])          # a sort by component all the same
        both = SS.segment_sum(terms[unstable], start)
        if not (SS.same_bits(both[:, 0], fixed["area"]).all() and SS.same_bits(both[:, 1], fixed["volume"]).all()):
            hits.append(tag)
    assert len([t for t in hits if t.startswith("triangle strip")]) == 4, hits   # (4095 terms over 16 binades, one component)
    # degenerate faces: both terms are exactly zero whatever the coordinates
    tag, v, f, _ = MC.corpus()[0]
    area, vol = _terms(tag, v, f, truth, MR.face_terms_exact)
    assert tag.startswith("edge path") and not area.any() and not vol.any()
