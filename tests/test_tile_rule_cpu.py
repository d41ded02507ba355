"""The per-object tile rule (``ops._tile_pad``) and the padding carrier (``ops.ObjectPad``) on the CPU: no library call.

A latent gradient is reduced over whole tiles of points per object -- 32 points (``ops.WAVE_TILE``) in the decoder / render / split
backward, 64 (``ops.DENSITY_TILE``) in the density backward.  ``_tile_pad(per_obj, unit, tile)`` is the smallest item count above
``per_obj`` whose ``unit`` points each fill whole tiles, 0 when ``per_obj`` already does; it is held here to that definition and to the
three formulas it replaced, restated literally."""
import math

import pytest
import torch

from supnerf_amd import ops

PER_OBJ = range(1, 261)
UNITS = (1, 2, 3, 4, 7, 8, 16, 32, 64, 128)
TILES = (32, 64)


def test_constants_are_the_kernels_tiles():
    assert (ops.WAVE_TILE, ops.DENSITY_TILE) == TILES


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("unit", UNITS)
def test_tile_pad_is_the_least_count_of_whole_tiles(unit, tile):
    for per_obj in PER_OBJ:
        r = ops._tile_pad(per_obj, unit, tile)
        whole = per_obj * unit % tile == 0
        assert (r == 0) == whole, (per_obj, unit, tile, r)
        if not whole:
            assert r > per_obj, (per_obj, unit, tile, r)
            assert r * unit % tile == 0, (per_obj, unit, tile, r)
            assert all(k * unit % tile for k in range(per_obj + 1, r)), (per_obj, unit, tile, r)


def parent_tile_pad(per_obj, unit=1):
    if (per_obj * unit) % 32 == 0:
        return 0
    step = 32 // math.gcd(32, unit)
    return -(-per_obj // step) * step


@pytest.mark.parametrize("unit", UNITS)
def test_tile_pad_equals_the_32_point_rule_it_had(unit):
    for per_obj in PER_OBJ:
        assert ops._tile_pad(per_obj, unit) == ops._tile_pad(per_obj, unit, 32) == parent_tile_pad(per_obj, unit), (per_obj, unit)


def test_tile_pad_equals_the_two_64_point_forms_it_replaces():
    for n in PER_OBJ:
        r = ops._tile_pad(n, 1, 64)
        assert r == (-(-n // 64) * 64 if n % 64 else 0), n          # DensityPoints, RaySurface
        assert (r or n) == -(-n // 64) * 64, n                      # iso_surface_points' rounding
    assert (ops._tile_pad(0, 1, 64) or 0) == -(-0 // 64) * 64       # (an empty surface stays empty)


@pytest.mark.parametrize("n_pad", [0, 8])
def test_object_pad_pads_and_strips_per_object_rows(n_pad):
    B, n = 3, 5
    pad = ops.ObjectPad(B, n, n_pad)
    assert tuple(pad) == (B, n, n_pad)
    b_, n_, p_ = pad
    assert (b_, n_, p_) == (B, n, n_pad)
    assert pad.pad(None) is None and pad.strip(None) is None
    for shape in ((B * n,), (B * n, 3), (B * n, 2, 4)):
        t = torch.arange(1, 1 + math.prod(shape), dtype=torch.float32).reshape(shape)
        padded = pad.pad(t)
        if n_pad == 0:
            assert padded is t and pad.strip(t) is t
            continue
        assert padded.shape == (B * n_pad, *shape[1:])
        rows = padded.reshape(B, n_pad, *shape[1:])
        assert torch.equal(rows[:, :n], t.reshape(B, n, *shape[1:]))
        assert not rows[:, n:].any()
        assert torch.equal(padded, ops._pad_rows(t, B, n, n_pad))
        assert torch.equal(pad.strip(padded), t)
        assert torch.equal(pad.strip(padded), ops._unpad_rows(padded, B, n, n_pad))
