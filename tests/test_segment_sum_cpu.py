"""tests/segment_sum_restatement.py against itself: on the inputs test_segment_sum_gpu.py feeds the kernels, the stated order gives other
bits than a sequential sum, than numpy's pairwise sum, than a slab of 4095 and than a lane stride of 32 -- so a kernel that summed in one
of those orders would not pass there.  And the one exported slab bound, without a GPU."""
import numpy as np

import segment_sum_restatement as SS


def test_hand_sums():
    """Small enough to follow by hand: one thread per term, then the tree's pairs; 257 terms put two on thread 0."""
    start = np.array([0, 0, 1, 4, 261])
    x = np.concatenate([[3.0], [1.0, 2.0 ** -53, 2.0 ** -53], np.ones(257) * 2.0 ** -53])
    x[4] = 1.0                                                    # (segment 3: term 0 is 1, 256 more of 2^-53)
    got = SS.segment_sum(x, start)
    assert got.shape == (4,) and got[0] == 0.0 and got[1] == 3.0
    # thread 0 holds 1, threads 1 and 2 hold 2^-53: the tree adds s[1] to s[0] (k = 1) after s[2] went to s[0] (k = 2): 1 twice, not 1 + 2^-52
    assert got[2] == 1.0 and (1.0 + 2.0 ** -53) + 2.0 ** -53 == 1.0 and 1.0 + (2.0 ** -53 + 2.0 ** -53) > 1.0
    # thread 0 adds terms 0 and 256: 1 + 2^-53 = 1, and 1 again with thread 128's 2^-53 (k = 128); the other 254 arrive in exact steps
    assert got[3] == 1.0 + 254 * 2.0 ** -53 and np.cumsum(x[4:261])[-1] == 1.0
    two = SS.segment_sum(np.stack([x, -x], 1), start)
    assert two.shape == (4, 2) and np.array_equal(two[:, 0], got) and np.array_equal(two[:, 1], -got)


def test_the_inputs_tell_orders_apart():
    x, start = SS.inputs()["area"], SS.starts(SS.LENGTHS)
    assert len(SS.LENGTHS) == 14 and x.shape == (start[-1],) and x.dtype == np.float64
    stated = SS.segment_sum(x, start)
    segs = [x[start[c]:start[c + 1]] for c in range(len(SS.LENGTHS))]
    long = np.array(SS.LENGTHS) >= 255
    sequential = np.array([np.cumsum(s)[-1] if len(s) else 0.0 for s in segs])
    pairwise = np.array([np.sum(s) for s in segs])
    slab_4095 = SS.segment_sum(x, start, slab=4095)
    differs = {name: ~SS.same_bits(stated, other) for name, other in (("sequential", sequential), ("np.sum", pairwise), ("slab 4095", slab_4095))}
    # a lane stride of 32 reorders three slab sums of the two segments past 64 slabs and nothing else, which rounds alike more often than
    # not: it shows on the 16-channel attributes (2 x 16 chances), not on one channel of terms
    wide, wstart = SS.inputs()["attributes"][16].astype(np.float64), SS.starts(SS.LENGTHS[1:])
    differs["lane stride 32"] = ~SS.same_bits(SS.segment_sum(wide, wstart), SS.segment_sum(wide, wstart, lane_stride=32))
    print({name: f"{int(d.sum())} of {d.size}" for name, d in differs.items()})
    assert differs["sequential"][long].all()
    assert differs["np.sum"][long].sum() >= long.sum() - 1
    assert differs["slab 4095"].any() and differs["lane stride 32"].any()
    # what must not differ: up to two terms every order is the same sum; the mutants are the stated order below their seams
    assert not differs["sequential"][:3].any() and not differs["slab 4095"][:6].any() and not differs["lane stride 32"][:11].any()
    # a segment alone gives what it gives among the others
    for c in (3, 8, 13):
        assert SS.same_bits(SS.segment_sum(segs[c], np.array([0, len(segs[c])])), stated[c:c + 1]).all()


def test_slab_layout():
    ids = np.array([2, 0, 2, 2, 5, 0])
    order, start, slabs = SS.segments(ids, 6)
    assert order.tolist() == [1, 5, 0, 2, 3, 4] and start.tolist() == [0, 2, 2, 5, 5, 5, 6] and slabs.tolist() == [0, 1, 1, 2, 2, 2, 3]
    _, start, slabs = SS.segments(np.repeat(np.arange(4), [4096, 4097, 0, 8193]), 4)
    assert np.diff(start).tolist() == [4096, 4097, 0, 8193] and slabs.tolist() == [0, 1, 3, 3, 6]


def test_one_exported_bound():
    import supnerf_amd as A  # noqa: F401
    from supnerf_amd import _lib, ops
    lib = _lib.lib()
    assert "snr_segment_slab_bound" in _lib.exported_symbols() and ops.MESH_SLAB == SS.SLAB
    assert lib.snr_segment_slab_bound(5, 10000) == 5 + 10000 // SS.SLAB and lib.snr_segment_slab_bound(4, -1) == 0
    for n_segments, lengths in ((4, [4096, 4097, 0, 8193]), (14, SS.LENGTHS)):          # the bound covers the layout's slab count
        assert lib.snr_segment_slab_bound(n_segments, sum(lengths)) >= sum(-(-n // SS.SLAB) for n in lengths)
    for gone in ("snr_mesh_slab_bound", "snr_simplify_slab_bound"):
        assert gone not in _lib.exported_symbols() and not hasattr(lib, gone)
