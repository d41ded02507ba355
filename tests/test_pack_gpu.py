"""GPU test of the packed decoder-weight buffer itself: ``ops.pack_weights`` against the numpy restatement of the format
(tests/pack_restatement.py), byte for byte -- every float of the buffer is defined by the format, so there is no tolerance.

Random decoders (nn.Linear's init) at four block counts; (8, 8) runs in exact fp32 only, its split streams are packed all the same.  Planted
into every weight tensor: -0 and +0, a value beyond the fp16 range on either side (the forward split stream clamps, the backward one does
not), one below the fp16 subnormal range (its forward pieces are both zero) and one whose fp16 high piece is exact (low piece zero); the last
of them sits on the tensor's last row and column, next to the padding."""
import numpy as np
import pytest

import pack_restatement as R
from oracle import supnerf_oracle as O
from oracle_bands import amd, dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

PLANTED = ((0, -0.0), (1, 0.0), (2, 1.0e5), (3, 1.0e-9), (4, 0.5), (-1, -7.0e4))


@pytest.mark.parametrize("blocks", [(0, 0), (3, 1), (1, 2), (8, 8)], ids=lambda b: f"{b[0]}_{b[1]}")
def test_packed_buffer_is_the_documented_image(amd, dev, blocks):
    sb, tb = blocks
    params = O.init_decoder_params(sb, tb, seed=17 + 10 * sb + tb)
    for name, t in params.items():
        if name.endswith(".weight"):
            for at, value in PLANTED:
                t.view(-1)[at] = value
    got = amd.ops.pack_weights({k: v.to(dev) for k, v in params.items()}, sb, tb).cpu().numpy().view(np.uint8)
    sections = R.packed_sections({k: v.numpy() for k, v in params.items()}, sb, tb)
    off = 0
    for name, want in sections:
        part = got[off:off + want.size]
        assert part.size == want.size, f"the buffer ends inside section {name}: {got.size} bytes, the section ends at {off + want.size}"
        bad = np.flatnonzero(part != want)
        assert bad.size == 0, (f"section {name} (bytes {off} .. {off + want.size}): {bad.size} bytes differ, the first at offset {bad[0]} of the "
                               f"section: got {part[bad[0]]:#04x}, the format says {want[bad[0]]:#04x}")
        off += want.size
    assert off == got.size, f"the buffer has {got.size} bytes, the format's sections {off}"
    assert np.array_equal(got, np.concatenate([b for _, b in sections]))
