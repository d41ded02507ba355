"""The fixed-order float64 segmented sum on the MI355X, bit for bit: every kernel that sums by it -- ``snr_mesh_segment_sum``,
``snr_simplify_attributes`` with 1, 3 and 16 channels, ``snr_simplify_positions`` with mean placement -- against
tests/segment_sum_restatement.py on segments of 0 to 65 * 4096 + 1 terms (every seam of the order), through the C ABI with every scratch
and output buffer between NaN guard bands.  Equal bits, no tolerance: the library is built with -ffp-contract=off, so float64 additions
in the stated order are the same operations here and there.  test_segment_sum_cpu.py shows that these inputs tell the stated order from a
sequential sum, numpy's pairwise sum, a slab of 4095 and a lane stride of 32."""
import numpy as np
import pytest
import torch

import segment_sum_restatement as SS
from oracle_bands import amd, dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

NAN = float("nan")
I64, F64, F32 = torch.int64, torch.float64, torch.float32


def _up(a, dev, dtype=None):  # noqa: F811
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(dev)


def _layout(lengths, dev):  # noqa: F811
    """(seg_start, slab_offset) on the device and the number of segments, of sorted segments of these lengths."""
    _, start, slabs = SS.segments(np.repeat(np.arange(len(lengths)), lengths), len(lengths))
    return _up(start, dev, I64), _up(slabs, dev, I64), len(lengths)


def _mesh_segment_sum(amd, dev, area_t, vol_t, lengths):  # noqa: F811
    """``snr_mesh_segment_sum`` over sorted terms of these segment lengths: (area, volume) as numpy, guard bands checked."""
    P, lib = amd.ops._ptr, amd._lib.lib()
    seg, slab, nC = _layout(lengths, dev)
    nF = int(sum(lengths))
    n_slabs = int(lib.snr_segment_slab_bound(nC, nF))
    part_full, part = SS.banded(n_slabs * 2, F64, dev, NAN)
    area_full, area = SS.banded(nC, F64, dev, NAN)
    vol_full, vol = SS.banded(nC, F64, dev, NAN)
    a, v = (_up(area_t, dev), _up(vol_t, dev)) if nF else (None, None)
    assert lib.snr_mesh_segment_sum(P(a, F64), P(v, F64), P(seg, I64), P(slab, I64), nC, nF, P(part, F64), n_slabs, P(area, F64), P(vol, F64),
                                    amd.ops._stream(dev)) == 0
    torch.cuda.synchronize()
    assert SS.bands_intact(part_full, n_slabs * 2, NAN) and SS.bands_intact(area_full, nC, NAN) and SS.bands_intact(vol_full, nC, NAN)
    return area.cpu().numpy(), vol.cpu().numpy()


def test_mesh_segment_sum_has_the_bits_of_the_stated_order(amd, dev):  # noqa: F811
    x = SS.inputs()
    start = SS.starts(SS.LENGTHS)
    want = SS.segment_sum(np.stack([x["area"], x["volume"]], 1), start)
    area, vol = _mesh_segment_sum(amd, dev, x["area"], x["volume"], SS.LENGTHS)          # all 14 segments in one call
    assert SS.same_bits(area, want[:, 0]).all() and SS.same_bits(vol, want[:, 1]).all(), (area, vol, want)
    for c, n in enumerate(SS.LENGTHS):                                                   # and a segment per call
        cut = slice(start[c], start[c + 1])
        area, vol = _mesh_segment_sum(amd, dev, x["area"][cut], x["volume"][cut], [n])
        assert SS.same_bits(area, want[c:c + 1, 0]).all() and SS.same_bits(vol, want[c:c + 1, 1]).all(), (n, area, vol, want[c])


@pytest.fixture(scope="module")
def clusters(dev):  # noqa: F811
    """The vertex segments of 13 clusters with SS.LENGTHS[1:] members, in the order of a fixed permutation."""
    x = SS.inputs()
    seg, slab, nC = _layout(x["members"], dev)
    return {"order": _up(x["vert_order"], dev), "seg": seg, "slab": slab, "nC": nC, "nV": int(sum(x["members"])),
            "count": np.array(x["members"], np.float64)}


def _unsorted(rows, order):
    """Per-vertex rows whose sorted list (row i = vertex order[i]) is ``rows``."""
    out = np.empty_like(rows)
    out[order] = rows
    return out


@pytest.mark.parametrize("channels", [1, 3, 16])
def test_attribute_means_have_the_bits_of_the_stated_order(amd, dev, clusters, channels):  # noqa: F811
    P, lib = amd.ops._ptr, amd._lib.lib()
    x, c = SS.inputs(), clusters
    rows = x["attributes"][channels]
    sum64 = SS.segment_sum(rows.astype(np.float64), SS.starts(x["members"]))
    want = (sum64 / c["count"][:, None]).astype(np.float32)
    att = _up(_unsorted(rows, x["vert_order"]), dev)
    n_slabs = int(lib.snr_segment_slab_bound(c["nC"], c["nV"]))
    part_full, part = SS.banded(n_slabs * channels, F64, dev, NAN)
    out_full, out = SS.banded(c["nC"] * channels, F32, dev, NAN)
    assert lib.snr_simplify_attributes(P(att), channels, c["nV"], P(c["order"], I64), P(c["seg"], I64), P(c["slab"], I64), c["nC"],
                                       P(part, F64), n_slabs, P(out), amd.ops._stream(dev)) == 0
    torch.cuda.synchronize()
    assert SS.bands_intact(part_full, n_slabs * channels, NAN) and SS.bands_intact(out_full, c["nC"] * channels, NAN)
    got = out.cpu().numpy().reshape(-1, channels)
    assert SS.same_bits(got, want).all(), (channels, np.argwhere(~SS.same_bits(got, want)))


def test_mean_positions_have_the_bits_of_the_stated_order(amd, dev, clusters):  # noqa: F811
    P, lib = amd.ops._ptr, amd._lib.lib()
    x, c = SS.inputs(), clusters
    sum64 = SS.segment_sum(x["verts"].astype(np.float64), SS.starts(x["members"]))
    want = (sum64 / c["count"][:, None]).astype(np.float32)
    verts = _up(_unsorted(x["verts"], x["vert_order"]), dev)
    voff = _up(np.array([0, c["nV"]]), dev, I64)
    cell, origin = torch.ones(1, device=dev), torch.zeros(1, 3, device=dev)               # (mean placement reads neither)
    n_slabs = int(lib.snr_segment_slab_bound(c["nC"], c["nV"]))
    part_full, part = SS.banded(n_slabs * 3, F64, dev, NAN)
    out_full, out = SS.banded(c["nC"] * 3, F32, dev, NAN)
    assert lib.snr_simplify_positions(P(verts), None, P(voff, I64), None, P(cell), P(origin), 1, c["nV"], 0, P(c["order"], I64),
                                      P(c["seg"], I64), P(c["slab"], I64), None, None, None, c["nC"], 0, P(part, F64), n_slabs, None, 0,
                                      P(out), amd.ops._stream(dev)) == 0
    torch.cuda.synchronize()
    assert SS.bands_intact(part_full, n_slabs * 3, NAN) and SS.bands_intact(out_full, c["nC"] * 3, NAN)
    got = out.cpu().numpy().reshape(-1, 3)
    assert SS.same_bits(got, want).all(), np.argwhere(~SS.same_bits(got, want))
