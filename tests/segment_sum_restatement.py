"""The fixed-order float64 segmented sum of include/supnerf_hip.h ("Fixed-order segmented sums"), restated in numpy float64, and the slab
layout its entry points take.  The library is built with -ffp-contract=off and adds nothing atomically, so IEEE float64 additions in the
same order give the same bits here as on the device: tests compare with ``==`` on the bit patterns, not with a tolerance."""
import functools

import numpy as np

SLAB, THREADS, LANES = 4096, 256, 64
# segment lengths at every seam of the order: the thread stride, the slab, two slabs, the lane stride (64 slabs) and past it
LENGTHS = (0, 1, 2, 255, 256, 257, 4095, 4096, 4097, 8192, 8193, 64 * 4096, 64 * 4096 + 1, 65 * 4096 + 1)


def draw(rng, lengths, *channels):
    """Sorted terms (sum lengths, *channels) float64, segment after segment from the one ``rng``: a normal deviate times a power of two
    over 40 binades each, so that almost every change of the order changes the rounded sum."""
    return np.concatenate([rng.standard_normal((n,) + channels) * 2.0 ** rng.integers(-20, 21, (n,) + channels) for n in lengths])


def starts(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def inputs():
    """What test_segment_sum_gpu.py feeds the kernels and test_segment_sum_cpu.py tells orders apart on, drawn once from default_rng(7):
    ``area`` and ``volume`` terms over all of LENGTHS; fp32 ``attributes`` (1, 3 and 16 channels) and ``verts`` over LENGTHS without the
    empty one (a cluster has a member), in sorted order -- row i belongs to vertex ``vert_order[i]``."""
    rng = np.random.default_rng(7)
    out = {"area": draw(rng, LENGTHS), "volume": draw(rng, LENGTHS), "members": LENGTHS[1:]}
    out["attributes"] = {C: draw(rng, LENGTHS[1:], C).astype(np.float32) for C in (1, 3, 16)}
    out["verts"] = draw(rng, LENGTHS[1:], 3).astype(np.float32)
    out["vert_order"] = np.random.default_rng(11).permutation(sum(LENGTHS[1:])).astype(np.int64)
    return out


def segments(ids, n, slab=SLAB):
    """(order, seg_start, slab_offset) of items with segment ids ``ids`` in [0, n): the stable sort by segment, where each segment starts
    in the sorted list, and the exclusive scan of ceil(length / slab)."""
    order = np.argsort(ids, kind="stable")
    start = np.searchsorted(ids[order], np.arange(n + 1))
    slabs = np.concatenate([[0], np.cumsum((np.diff(start) + slab - 1) // slab)])
    return order, start, slabs


def _strided_then(x, width, stride, combine):
    """Slot t of ``width`` starts from 0.0 and adds rows t, t + stride, ... of x (m, C) in that order; then ``combine`` over the slots."""
    acc = np.zeros((width, x.shape[1]))
    for r in range(0, len(x), stride):
        part = x[r:r + stride]
        acc[:len(part)] += part
    k = width // 2
    while k:
        acc = combine(acc, k)
        k //= 2
    return acc[0]


def _tree(acc, k):              # s[t] += s[t + k] for t < k
    acc[:k] += acc[k:2 * k]
    return acc


def _butterfly(acc, k):         # every lane: a += shfl_xor(a, k)
    return acc + acc[np.arange(len(acc)) ^ k]


def segment_sum(terms, seg_start, slab=SLAB, lane_stride=LANES):
    """out (n_segments, ...) float64 of ``terms`` (n, ...) float64 sorted by segment, segment c at [seg_start[c], seg_start[c + 1]).
    ``slab`` and ``lane_stride`` other than the header's plant a wrong order (what a test must be able to tell apart)."""
    x = np.asarray(terms, np.float64).reshape(len(terms), -1)
    out = np.zeros((len(seg_start) - 1, x.shape[1]))
    for c in range(len(out)):
        seg = x[seg_start[c]:seg_start[c + 1]]
        partial = [_strided_then(seg[i:i + slab], THREADS, THREADS, _tree) for i in range(0, len(seg), slab)]
        out[c] = _strided_then(np.reshape(partial, (-1, x.shape[1])), LANES, lane_stride, _butterfly)
    return out.reshape((len(out),) + np.shape(terms)[1:])


def same_bits(a, b):
    """Per element: do two float64 (or two float32) arrays hold the same bit patterns?"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    bits = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return a.view(bits) == b.view(bits)


def banded(n, dtype, dev, fill, band=64):
    """(the whole buffer, its middle n elements) of a torch buffer with ``band`` elements of ``fill`` on either side."""
    import torch
    full = torch.full((n + 2 * band,), fill, dtype=dtype, device=dev)
    return full, full[band:band + n]


def bands_intact(full, n, fill, band=64):
    import torch
    lo, hi = full[:band], full[band + n:]
    ok = (lambda t: bool(torch.isnan(t).all())) if fill != fill else (lambda t: bool((t == fill).all()))
    return ok(lo) and ok(hi)
