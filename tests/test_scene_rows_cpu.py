"""CPU tests of the scene sample kernels' rules: the restatement (tests/scene_rows_restatement.py) against ``scene.scene_ray_rows`` + the
sample lines of ``scene.render_scene_batch`` in float64, ``scene.scene_rois`` against the rois inside ``scene.scene_rays``, the C ABI's
new symbols and argument checks (no launch is made), and the operators' own checks."""
import ctypes as C
import os
import re

import pytest
import torch

import scene_rows_restatement as R
from oracle_bands import amd  # noqa: F401  (a fixture)

S = 16


@pytest.fixture(scope="module")
def scene(golden):
    g = golden("scene")
    H, W = int(g["H"]), int(g["W"])
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return g, H, W, torch.stack([xs.reshape(-1), ys.reshape(-1)], 1)          # every pixel, row-major like the table


def perturbed(amd, poses, seed):
    """The fixture's poses turned by ~0.05 rad and moved by ~0.1 (seed 0: the fixture's own)."""
    poses = poses.double()
    if seed == 0:
        return poses
    gen = torch.Generator().manual_seed(seed)
    dR = amd.driver.axis_angle_to_matrix(torch.randn(poses.shape[0], 3, generator=gen).double() * 0.05)
    return torch.cat([dR @ poses[:, :, :3], poses[:, :, 3:] + torch.randn(poses.shape[0], 3, 1, generator=gen).double() * 0.1], dim=2)


@pytest.mark.parametrize("rend_aabb,shapenet,scale", [(True, True, 1.0), (False, False, 0.7)])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_restatement_equals_existing_functions(amd, scene, seed, rend_aabb, shapenet, scale):
    """float64 on all 4800 pixels: identical hit flags; on hit pairs the same points, directions and depths to float64 rounding; on the
    others the restatement's stated constants and the existing route's depth -1."""
    g, H, W, pixels = scene
    poses = perturbed(amd, g["obj_poses"], seed)
    Nb = poses.shape[0]
    jitter = torch.rand(pixels.shape[0] * Nb, S, generator=torch.Generator().manual_seed(10 + seed), dtype=torch.float64)
    K = g["K"]
    want = R.existing_route(amd.scene, poses, g["obj_wlh"], K, pixels, H, W, jitter, S, scale, rend_aabb, shapenet)
    rois = amd.scene.scene_rois(poses, g["obj_wlh"], K, H, W)
    got = R.scene_samples(R.cam2obj_of(poses), g["obj_wlh"], rois, pixels, (K[0, 0], K[1, 1], K[0, 2], K[1, 2]), jitter, S, scale, rend_aabb, shapenet)
    assert got["xyz"].dtype == torch.float64
    assert torch.equal(got["hit"], want["hit"])
    assert 0 < int(got["hit"].sum()) < got["hit"].numel() and bool((got["covered"] & ~got["hit"]).any()) == rend_aabb
    m3, m1 = R.pair_mask(got["hit"], S)
    for k, m in (("xyz", m3), ("viewdir", m3), ("z_vals", m1)):
        err = float((got[k] - want[k])[m].abs().max())
        print(f"seed {seed} {k}: {err:.2e}")
        assert err < 1e-12, (k, err)
    assert bool((got["z_vals"][~m1] == -1).all()) and bool((want["z_vals"][~m1] == -1).all())
    assert bool((got["xyz"][~m3] == 0).all())
    assert torch.equal(got["viewdir"][~m3].view(-1, 3), torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64).expand(int((~m3).sum()) // 3, 3))
    assert torch.equal(got["valid"], got["hit"].any(1))


def test_restatement_fixture_counts(amd, scene):
    """What the GPU tests' exclusion cap rests on: float64 against fp32 on the fixture, 0 flag differences and no thin hit."""
    g, H, W, pixels = scene
    K = g["K"]
    Kvec = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    rois = amd.scene.scene_rois(g["obj_poses"], g["obj_wlh"], K, H, W)
    o64 = R.scene_samples(R.cam2obj_of(g["obj_poses"].double()), g["obj_wlh"], rois, pixels, Kvec, None, S)
    o32 = R.scene_samples(R.cam2obj_of(g["obj_poses"].float()), g["obj_wlh"], rois, pixels, Kvec, None, S)
    assert int(o64["hit"].sum()) == 1627 and torch.equal(o64["hit"], o32["hit"])
    assert int((o64["hit"] & (o64["gap"] < 1e-3)).sum()) == 0
    print(f"hit share: {float(o64['hit'].float().mean()):.3f} of all pairs, {float(o64['hit'].sum()) / float(o64['covered'].sum()):.3f} of the covered ones")


@pytest.mark.parametrize("manipulation", [(0.0, 0.0, 0.0), (0.3, -0.1, 0.5)])
def test_scene_rois_are_scene_rays_rois(amd, scene, manipulation):
    """The roi of every object is the box of pixels whose row ``scene_rays`` filled."""
    g, H, W, _ = scene
    table, _, _ = amd.scene.scene_rays(g["obj_poses"], g["obj_wlh"], g["K"], H, W, manipulation, rend_aabb=False)
    rois = amd.scene.scene_rois(g["obj_poses"], g["obj_wlh"], g["K"], H, W, manipulation)
    assert rois.dtype == torch.int32 and rois.shape == (g["obj_poses"].shape[0], 4)
    for b in range(rois.shape[0]):
        filled = ~(table[:, :, b] == -1).all(-1)                               # (H,W)
        ys, xs = torch.nonzero(filled, as_tuple=True)
        assert ys.numel() > 0
        assert rois[b].tolist() == [int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1]
        assert int(filled.sum()) == (int(xs.max()) + 1 - int(xs.min())) * (int(ys.max()) + 1 - int(ys.min()))
    # the host formula itself, line for line
    S_ = amd.scene
    poses = g["obj_poses"].float().clone()
    poses[:, :, 3] += torch.tensor(manipulation).unsqueeze(0)
    uv = S_.view_points_batch(S_.corners_of_box_batch(poses, g["obj_wlh"].float()), g["K"].float().unsqueeze(0).repeat(poses.shape[0], 1, 1))
    raw = torch.stack([uv[:, 0].min(dim=1)[0], uv[:, 1].min(dim=1)[0], uv[:, 0].max(dim=1)[0], uv[:, 1].max(dim=1)[0]], dim=1).type(torch.int32)
    want = torch.stack([raw[:, 0].clamp(min=0), raw[:, 1].clamp(min=0), raw[:, 2].clamp(max=W - 1), raw[:, 3].clamp(max=H - 1)], 1)
    assert torch.equal(rois, want)
    # an object behind the image's edge: a dead roi
    far_left = g["obj_poses"].clone()
    far_left[:, 0, 3] -= 1000.0
    dead = amd.scene.scene_rois(far_left, g["obj_wlh"], g["K"], H, W)
    assert bool((dead[:, 2] <= dead[:, 0]).all())


# ------------------------------------------------------------------------------------------------ C ABI
NEW = ("snr_scene_samples_fwd", "snr_scene_samples_bwd", "snr_scene_gather_fwd", "snr_scene_gather_bwd")


def test_abi_version_and_symbols(amd):
    hdr = open(os.path.join(os.path.dirname(amd.__file__), "..", "include", "supnerf_hip.h")).read()
    assert amd._lib.header_abi_version() >= 17
    lib = amd._lib.lib()
    assert lib.snr_abi_version() == amd._lib.header_abi_version()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in amd._lib.exported_symbols()
        assert getattr(lib, name) is not None
    assert lib.snr_scene_samples_bwd_ws_bytes(257, 3) == 2 * 3 * 12 * 8 and lib.snr_scene_samples_bwd_ws_bytes(0, 3) == 0


OK, E_ARG, E_WORKSPACE = 0, -1, -3
P_ = C.c_void_p(0x1000)      # never dereferenced on the host: every case below returns before a launch
N_ = C.c_void_p(0)
K4 = (100.0, 100.0, 40.0, 30.0)
#   cam2obj wlh rois pixels K jitter Nr Nb S scale aabb shapenet | xyz viewdir z hit valid stream
FWD_CASES = {
    "empty_all_null": ((N_, N_, N_, N_, *K4, N_, 0, 3, 16, 1.0, 1, 1, N_, N_, N_, N_, N_, N_), OK),
    "null_cam2obj": ((N_, P_, P_, P_, *K4, N_, 4, 3, 16, 1.0, 1, 1, P_, P_, P_, P_, N_, N_), E_ARG),
    "null_pixels": ((P_, P_, P_, N_, *K4, N_, 4, 3, 16, 1.0, 1, 1, P_, P_, P_, P_, N_, N_), E_ARG),
    "null_hit": ((P_, P_, P_, P_, *K4, N_, 4, 3, 16, 1.0, 1, 1, P_, P_, P_, N_, N_, N_), E_ARG),
    "negative_pixels": ((P_, P_, P_, P_, *K4, N_, -1, 3, 16, 1.0, 1, 1, P_, P_, P_, P_, N_, N_), E_ARG),
    "no_object": ((P_, P_, P_, P_, *K4, N_, 4, 0, 16, 1.0, 1, 1, P_, P_, P_, P_, N_, N_), E_ARG),
    "too_many_objects": ((P_, P_, P_, P_, *K4, N_, 4, 65536, 16, 1.0, 1, 1, P_, P_, P_, P_, N_, N_), E_ARG),
    "no_sample": ((P_, P_, P_, P_, *K4, N_, 4, 3, 0, 1.0, 1, 1, P_, P_, P_, P_, N_, N_), E_ARG),
}
#   ... | d_xyz d_viewdir d_z d_cam2obj ws ws_bytes stream
BWD_CASES = {
    "empty_all_null": ((N_, N_, N_, N_, *K4, N_, 0, 3, 16, 1.0, 1, 1, N_, N_, N_, N_, N_, 0, N_), OK),
    "null_out": ((P_, P_, P_, P_, *K4, N_, 4, 3, 16, 1.0, 1, 1, P_, P_, P_, N_, P_, 1 << 20, N_), E_ARG),
    "null_ws": ((P_, P_, P_, P_, *K4, N_, 4, 3, 16, 1.0, 1, 1, P_, P_, P_, P_, N_, 1 << 20, N_), E_ARG),
    "odd_ws": ((P_, P_, P_, P_, *K4, N_, 4, 3, 16, 1.0, 1, 1, P_, P_, P_, P_, C.c_void_p(0x1004), 1 << 20, N_), E_ARG),
    "small_ws": ((P_, P_, P_, P_, *K4, N_, 257, 3, 16, 1.0, 1, 1, P_, P_, P_, P_, P_, 2 * 3 * 12 * 8 - 1, N_), E_WORKSPACE),
    "no_sample": ((P_, P_, P_, P_, *K4, N_, 4, 3, 0, 1.0, 1, 1, P_, P_, P_, P_, P_, 1 << 20, N_), E_ARG),
}
#   in_sig in_rgb hit Nr Nb S out_sig out_rgb stream
GATHER_CASES = {
    "empty_all_null": ((N_, N_, N_, 0, 3, 16, N_, N_, N_), OK),
    "null_hit": ((P_, P_, N_, 4, 3, 16, P_, P_, N_), E_ARG),
    "no_output": ((P_, P_, P_, 4, 3, 16, N_, N_, N_), E_ARG),
    "output_without_input": ((N_, P_, P_, 4, 3, 16, P_, P_, N_), E_ARG),
    "no_sample": ((P_, P_, P_, 4, 3, 0, P_, P_, N_), E_ARG),
}


@pytest.mark.parametrize("fn,name", [("snr_scene_samples_fwd", n) for n in FWD_CASES] + [("snr_scene_samples_bwd", n) for n in BWD_CASES]
                         + [(f, n) for f in ("snr_scene_gather_fwd", "snr_scene_gather_bwd") for n in GATHER_CASES])
def test_argument_checks(amd, fn, name):
    args, want = {"snr_scene_samples_fwd": FWD_CASES, "snr_scene_samples_bwd": BWD_CASES}.get(fn, GATHER_CASES)[name]
    assert getattr(amd._lib.lib(), fn)(*args) == want


# ------------------------------------------------------------------------------------------------ operators
def test_operator_errors(amd):
    ops = amd.ops
    cam2obj, wlh = torch.eye(3, 4)[None].repeat(2, 1, 1), torch.ones(2, 3)
    rois = torch.tensor([[0, 0, 8, 8], [0, 0, 8, 8]], dtype=torch.int32)
    pixels = torch.tensor([[1, 1], [2, 3]], dtype=torch.int32)
    Kvec = (10.0, 10.0, 4.0, 4.0)
    good = (cam2obj, wlh, rois, pixels, Kvec, None, 4, 1.0, True, True)
    with pytest.raises(amd.SnrError, match="GPU"):
        ops.SceneSamples.apply(*good)

    def bad(i, v):
        a = list(good)
        a[i] = v
        with pytest.raises(amd.SnrError, match="scene_samples"):
            ops.SceneSamples.apply(*a)
    bad(0, cam2obj[:, :, :3]); bad(1, wlh[:1]); bad(2, rois[:1]); bad(2, rois.long()); bad(3, pixels.long()); bad(3, pixels[:, :1])
    bad(5, torch.zeros(3, 4)); bad(6, 0); bad(4, (1.0, 1.0, 1.0))
    hit = torch.ones(2, 2, dtype=torch.uint8)
    with pytest.raises(amd.SnrError, match="GPU"):
        ops.SceneGather.apply(torch.zeros(16), torch.zeros(16, 3), hit, 4)
    for args in ((torch.zeros(15), torch.zeros(16, 3), hit, 4), (torch.zeros(16), torch.zeros(16, 2), hit, 4),
                 (torch.zeros(16), torch.zeros(16, 3), hit.bool(), 4), (torch.zeros(16), torch.zeros(16, 3), hit, 0)):
        with pytest.raises(amd.SnrError, match="scene_gather"):
            ops.SceneGather.apply(*args)
