"""The return codes of the decoder's twelve C entry points (csrc/snr_decoder.hip) for calls that return before any device work, and the
workspace sizes.  The library loads without a GPU; pointers are null or a dummy address that the host never dereferences.

The ORDER of the checks inside an entry point is behaviour, quirks included: an empty ``snr_decoder_bwd`` succeeds with every pointer null
and with block counts and a precision that a non-empty call refuses, an empty ``snr_density_bwd`` with a null pointer does not; a null
pointer wins over a bad shape; an unknown precision is only seen by a call that has work to do.  The expected values were recorded from the
library before the entry points moved into one file.

Base call: 64 points, 64 per object, 3/1 blocks, fp32, all pointers set, no latent gradient; render: 64 rays of 64 samples, shared depths.
The density lattice and brick entry points are covered by tests/test_narrow_band_cpu.py."""
import ctypes as C

import pytest

import supnerf_amd as A

OK, E_ARG, E_SHAPE, E_WORKSPACE, E_UNSUPPORTED = 0, -1, -2, -3, -5
P = C.c_void_p(0x1000)      # never dereferenced on the host: every case below returns before a launch
N = None
FP32, SPLIT, METRIC_Z, Z_BOX = 0, 1, 2, 3


def _lib():
    return A._lib.lib()


def _ra(**kw):
    a = A._lib.RenderArgs()
    d = dict(rays_o=0x1000, rays_d=0x1000, t_vals=0x1000, xyz_div=0x1000, z_scale=0x1000, latent=0x1000, packed=0x1000, z_mode=0, flags=0,
             n_rays=64, rays_per_obj=64, n_samples=64, shape_blocks=3, texture_blocks=1, precision=FP32)
    d.update(kw)
    for k, v in d.items():
        setattr(a, k, v)
    return C.byref(a)


# snr_decoder_fwd(xyz, viewdir, latent, packed, P, ppo, sb, tb, sigmas, rgbs, masks, activations, precision, stream)
DECODER_FWD = {
    "null_xyz": ((N, P, P, P, 64, 64, 3, 1, P, P, N, N, FP32, N), E_ARG),
    "activations_without_masks": ((P, P, P, P, 64, 64, 3, 1, P, P, N, P, FP32, N), E_ARG),
    "blocks_9": ((P, P, P, P, 64, 64, 9, 1, P, P, N, N, FP32, N), E_ARG),
    "negative_points": ((P, P, P, P, -1, 64, 3, 1, P, P, N, N, FP32, N), E_ARG),
    "bad_precision": ((P, P, P, P, 64, 64, 3, 1, P, P, N, N, 7, N), E_ARG),
    "ppo_0": ((P, P, P, P, 64, 0, 3, 1, P, P, N, N, FP32, N), E_SHAPE),
    "ppo_not_dividing": ((P, P, P, P, 64, 48, 3, 1, P, P, N, N, FP32, N), E_SHAPE),
    "null_and_bad_shape": ((N, P, P, P, 64, 48, 3, 1, P, P, N, N, FP32, N), E_ARG),
    "empty": ((P, P, P, P, 0, 64, 3, 1, P, P, N, N, FP32, N), OK),
    "empty_bad_precision": ((P, P, P, P, 0, 64, 3, 1, P, P, N, N, 7, N), OK),
    "split_unsupported_blocks": ((P, P, P, P, 64, 64, 5, 5, P, P, N, N, SPLIT, N), E_UNSUPPORTED),
    "split_unsupported_ppo": ((P, P, P, P, 70, 35, 3, 1, P, P, N, N, SPLIT, N), E_UNSUPPORTED),
}

# snr_decoder_bwd(xyz, viewdir, latent, packed, masks, sigmas, d_sigmas, d_rgbs, P, ppo, sb, tb, d_latent, d_xyz, d_viewdir, layer_grads,
#                 workspace, ws_bytes, precision, stream)
DECODER_BWD = {
    "empty_all_null": ((N, N, N, N, N, N, N, N, 0, 0, 9, 9, N, N, N, N, N, 0, 7, N), OK),
    "null_masks": ((P, P, P, P, N, P, P, P, 64, 64, 3, 1, N, P, P, N, N, 0, FP32, N), E_ARG),
    "blocks_9": ((P, P, P, P, P, P, P, P, 64, 64, 3, 9, N, P, P, N, N, 0, FP32, N), E_ARG),
    "bad_precision": ((P, P, P, P, P, P, P, P, 64, 64, 3, 1, N, P, P, N, N, 0, 7, N), E_ARG),
    "ppo_not_dividing": ((P, P, P, P, P, P, P, P, 64, 48, 3, 1, N, P, P, N, N, 0, FP32, N), E_SHAPE),
    "latent_ppo_48": ((P, P, P, P, P, P, P, P, 96, 48, 3, 1, P, P, P, N, P, 1 << 30, FP32, N), E_UNSUPPORTED),
    "latent_no_workspace": ((P, P, P, P, P, P, P, P, 64, 64, 3, 1, P, P, P, N, N, 0, FP32, N), E_WORKSPACE),
    "split_unsupported": ((P, P, P, P, P, P, P, P, 64, 64, 5, 5, N, P, P, N, N, 0, SPLIT, N), E_UNSUPPORTED),
}

# snr_density_fwd(xyz, latent, packed, P, ppo, sb, tb, sigmas, stream)
DENSITY_FWD = {
    "null_sigmas": ((P, P, P, 64, 64, 3, 1, N, N), E_ARG),
    "negative_blocks": ((P, P, P, 64, 64, -1, 1, P, N), E_ARG),
    "empty_null_xyz": ((N, P, P, 0, 64, 3, 1, P, N), E_ARG),
    "ppo_not_dividing": ((P, P, P, 64, 48, 3, 1, P, N), E_SHAPE),
    "empty": ((P, P, P, 0, 64, 3, 1, P, N), OK),
}

# snr_density_fwd_masks(xyz, latent, packed, P, ppo, sb, tb, sigmas, masks, stream)
DENSITY_FWD_MASKS = {
    "null_masks": ((P, P, P, 64, 64, 3, 1, P, N, N), E_ARG),
    "empty": ((P, P, P, 0, 64, 3, 1, P, P, N), OK),
}

# snr_density_bwd(xyz, latent, packed, masks, sigmas, d_sigmas, P, ppo, sb, tb, d_latent, d_xyz, workspace, ws_bytes, stream)
DENSITY_BWD = {
    "empty_all_null": ((N, N, N, N, N, N, 0, 64, 3, 1, N, N, N, 0, N), E_ARG),
    "null_d_sigmas": ((P, P, P, P, P, N, 64, 64, 3, 1, N, P, N, 0, N), E_ARG),
    "empty": ((P, P, P, P, P, P, 0, 64, 3, 1, N, N, N, 0, N), OK),
    "ppo_not_dividing": ((P, P, P, P, P, P, 64, 48, 3, 1, N, P, N, 0, N), E_SHAPE),
    "latent_ppo_96": ((P, P, P, P, P, P, 192, 96, 3, 1, P, P, P, 1 << 30, N), E_UNSUPPORTED),
    "latent_no_workspace": ((P, P, P, P, P, P, 128, 128, 3, 1, P, P, N, 0, N), E_WORKSPACE),
}

# snr_render_fwd(args, rgb, depth, acc, sigmas, rgbs, masks, stream): (args or None for a null pointer, then the outputs)
RENDER_FWD = {
    "null_args": (None, (P, P, P), E_ARG),
    "null_rays_o": (dict(rays_o=None), (P, P, P), E_ARG),
    "z_mode_4": (dict(z_mode=4), (P, P, P), E_ARG),
    "box_without_box_half": (dict(z_mode=Z_BOX), (P, P, P), E_ARG),
    "metric_z_without_z_scale": (dict(flags=METRIC_Z, z_scale=None), (P, P, P), E_ARG),
    "null_latent": (dict(latent=None), (P, P, P), E_ARG),
    "shape_blocks_9": (dict(shape_blocks=9), (P, P, P), E_ARG),
    "null_depth": (dict(), (P, N, P), E_ARG),
    "bad_precision": (dict(precision=7), (P, P, P), E_ARG),
    "rays_per_obj_48": (dict(rays_per_obj=48), (P, P, P), E_SHAPE),
    "box_48_samples": (dict(z_mode=Z_BOX, box_half=0x1000, n_samples=48), (P, P, P), E_UNSUPPORTED),
    "48_samples": (dict(n_samples=48), (P, P, P), E_UNSUPPORTED),
    "256_samples": (dict(n_samples=256), (P, P, P), E_UNSUPPORTED),
    "split_unsupported": (dict(shape_blocks=5, texture_blocks=5, precision=SPLIT), (P, P, P), E_UNSUPPORTED),
    "empty": (dict(n_rays=0), (P, P, P), OK),
    "empty_bad_precision": (dict(n_rays=0, precision=7), (P, P, P), OK),
}

# snr_render_bwd(args, sigmas, rgbs, masks, d_rgb, d_depth, d_acc, d_latent, d_rays_o, d_rays_d, d_t, workspace, ws_bytes, stream):
# (args or None, the arguments after args)
RENDER_BWD = {
    "null_args": (None, (P, P, P, P, P, P, N, P, P, N, N, 0, N), E_ARG),
    "null_saved_rgbs": (dict(), (P, N, P, P, P, P, N, P, P, N, N, 0, N), E_ARG),
    "bad_precision": (dict(precision=7), (P, P, P, P, P, P, N, P, P, N, N, 0, N), E_ARG),
    "empty_null_saved": (dict(n_rays=0), (N, N, N, P, P, P, N, P, P, N, N, 0, N), OK),
    "48_samples": (dict(n_samples=48), (P, P, P, P, P, P, N, P, P, N, N, 0, N), E_UNSUPPORTED),
    "d_t_with_shared_depths": (dict(), (P, P, P, P, P, P, N, P, P, P, N, 0, N), E_UNSUPPORTED),
    "latent_48_points_per_object": (dict(n_rays=6, rays_per_obj=3, n_samples=16), (P, P, P, P, P, P, P, P, P, N, P, 1 << 30, N), E_UNSUPPORTED),
    "split_unsupported": (dict(shape_blocks=5, texture_blocks=5, precision=SPLIT), (P, P, P, P, P, P, N, P, P, N, N, 0, N), E_UNSUPPORTED),
    "latent_no_workspace": (dict(), (P, P, P, P, P, P, P, P, P, N, N, 0, N), E_WORKSPACE),
}

POINT_ENTRIES = {"snr_decoder_fwd": DECODER_FWD, "snr_decoder_bwd": DECODER_BWD, "snr_density_fwd": DENSITY_FWD,
                 "snr_density_fwd_masks": DENSITY_FWD_MASKS, "snr_density_bwd": DENSITY_BWD}
RENDER_ENTRIES = {"snr_render_fwd": RENDER_FWD, "snr_render_bwd": RENDER_BWD}


@pytest.mark.parametrize("entry,case", [(e, c) for e, cases in POINT_ENTRIES.items() for c in cases])
def test_point_entry_return_codes(entry, case):
    args, want = POINT_ENTRIES[entry][case]
    assert getattr(_lib(), entry)(*args) == want


def test_decoder_bwd_refuses_a_workspace_one_byte_short():
    lib = _lib()
    short = lib.snr_decoder_bwd_ws_bytes(64, 64, 3, 1) - 1
    assert lib.snr_decoder_bwd(P, P, P, P, P, P, P, P, 64, 64, 3, 1, P, P, P, N, P, short, FP32, N) == E_WORKSPACE


@pytest.mark.parametrize("entry,case", [(e, c) for e, cases in RENDER_ENTRIES.items() for c in cases])
def test_render_entry_return_codes(entry, case):
    fields, rest, want = RENDER_ENTRIES[entry][case]
    a = None if fields is None else _ra(**fields)
    more = (N, N, N, N) if entry == "snr_render_fwd" else ()          # sigmas, rgbs, masks, stream
    assert getattr(_lib(), entry)(a, *rest, *more) == want


def test_workspace_sizes():
    lib = _lib()
    assert lib.snr_decoder_bwd_ws_bytes(64, 64, 3, 1) == 16640
    assert lib.snr_decoder_bwd_ws_bytes(1000, 0, 3, 1) == 139520
    assert lib.snr_decoder_bwd_ws_bytes(262144, 4096, 3, 1) == 34865408
    assert lib.snr_decoder_bwd_ws_bytes(0, 0, 0, 0) == 256
    assert lib.snr_render_bwd_ws_bytes(None) == 0
    assert lib.snr_render_bwd_ws_bytes(_ra(n_rays=4096, rays_per_obj=4096)) == 34636032          # 4096 rays x 64 samples, one object


def test_precision_supported():
    lib = _lib()
    assert lib.snr_precision_supported(FP32, 8, 8, 35) == 1
    assert lib.snr_precision_supported(FP32, 9, 1, 64) == 0
    assert lib.snr_precision_supported(SPLIT, 3, 1, 64) == 1
    assert lib.snr_precision_supported(SPLIT, 3, 2, 64) == 0
    assert lib.snr_precision_supported(7, 3, 1, 64) == 0
