"""CPU tests of the compact scene route's rules: the restatement (tests/scene_compact_restatement.py) pinned to tests/scene_rows_restatement.py
in float64, its slot and overflow rules, ``ops.scene_capacity``, the C ABI's new symbols and argument checks (no launch is made), the
operators' own checks and the misuse cases of ``scene.render_scene``."""
import ctypes as C
import os
import re

import pytest
import torch

import scene_compact_restatement as RC
import scene_rows_restatement as R
from oracle_bands import amd  # noqa: F401  (a fixture)
from test_scene_rows_gpu import make_case

EDGE_SHAPES = [(1, 300, 64), (8, 1025, 2), (3, 257, 1)]


def dense64(c):
    return R.scene_samples(R.cam2obj_of(c["poses"].double()), c["wlh"], c["rois"], c["pixels"], c["Kvec"], c["jitter"], c["S"], c["scale"],
                           c["rend_aabb"], c["shapenet"])


def fixture_case(amd, golden):
    g = golden("scene")
    H, W, S = int(g["H"]), int(g["W"]), 4
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    pixels = torch.stack([xs.reshape(-1), ys.reshape(-1)], 1)
    K = g["K"]
    Nb = g["obj_poses"].shape[0]
    return dict(poses=g["obj_poses"], wlh=g["obj_wlh"], rois=amd.scene.scene_rois(g["obj_poses"], g["obj_wlh"], K, H, W), pixels=pixels,
                Kvec=(float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])), S=S, scale=1.0, rend_aabb=True, shapenet=True,
                jitter=torch.rand(pixels.shape[0] * Nb, S, generator=torch.Generator().manual_seed(1)), Nb=Nb, Nr=pixels.shape[0])


def cases(amd, golden):
    return [(f"{s}", make_case(amd, *s, seed=sum(s))) for s in EDGE_SHAPES] + [("fixture", fixture_case(amd, golden))]


def test_edge_cases_are_what_the_gpu_tests_count_on(amd):
    """float64: (1,300,64) has 192 hits, 163 of them in the first 256-pixel slice; (8,1025,2) has 21 .. 151 per object.  No hit of the
    first grazes (slab gap below 1e-3), so the kernel's fp32-input flags there are the float64 ones."""
    o = dense64(make_case(amd, 1, 300, 64, seed=365))
    assert int(o["hit"].sum()) == 192 and int(o["hit"][:256].sum()) == 163 and int((o["hit"] & (o["gap"] < 1e-3)).sum()) == 0
    o = dense64(make_case(amd, 8, 1025, 2, seed=1035))
    n = o["hit"].sum(0)
    assert int(n.min()) == 21 and int(n.max()) == 151


def test_restatement_is_pinned_to_the_dense_one(amd, golden):
    """Compacting the dense float64 outputs and gathering back is the dense gather bit for bit; the points scatter back to the dense ones."""
    for name, c in cases(amd, golden):
        o = dense64(c)
        S, Nb, Nr = c["S"], c["Nb"], c["Nr"]
        hit = o["hit"]
        cap = RC.capacity(int(hit.sum(0).max()))
        comp = RC.scene_samples_compact(o, hit, cap, S)
        assert comp["xyz"].shape == (Nb * cap, S, 3) and comp["xyz"].dtype == torch.float64 and torch.equal(comp["kept"], hit), name
        assert torch.equal(comp["z_vals"], o["z_vals"]), name
        assert torch.equal(RC.scatter_rows(comp["xyz"], comp["slot"], comp["kept"], 0.0), o["xyz"]), name
        assert torch.equal(RC.scatter_rows(comp["viewdir"], comp["slot"], comp["kept"], [0.0, 0.0, 1.0]).abs(), o["viewdir"].abs()), name
        gen = torch.Generator().manual_seed(3)
        sig = torch.randn(Nb * Nr * S, generator=gen, dtype=torch.float64)
        rgb = torch.rand(Nb * Nr * S, 3, generator=gen, dtype=torch.float64)
        sig_c = RC.compact_rows(sig.view(-1, S), comp["slot"], comp["kept"], cap, 7.0)          # (what the decoder makes of padding is arbitrary)
        rgb_c = RC.compact_rows(rgb.view(-1, S, 3), comp["slot"], comp["kept"], cap, 7.0)
        got, want = RC.gather_compact(sig_c, rgb_c, comp["slot"], comp["kept"], S), R.gather(sig, rgb, hit, S)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), name
        # the backward: the transpose of the forward, exact zeros on padding
        d_s, d_r = torch.randn(Nr, Nb * S, generator=gen, dtype=torch.float64), torch.randn(Nr, Nb * S, 3, generator=gen, dtype=torch.float64)
        a, b = sig_c.clone().requires_grad_(), rgb_c.clone().requires_grad_()
        out = RC.gather_compact(a, b, comp["slot"], comp["kept"], S)
        ga, gb = torch.autograd.grad((out[0] * d_s).sum() + (out[1] * d_r).sum(), (a, b))
        ha, hb = RC.gather_compact_bwd(d_s, d_r, comp["pair_of_slot"], S)
        assert torch.equal(ga.reshape(-1), ha) and torch.equal(gb.reshape(-1, 3), hb), name
        pad = (comp["pair_of_slot"] < 0).reshape(-1)
        assert bool((ha.view(-1, S)[pad] == 0).all()) and bool((hb.view(-1, S, 3)[pad] == 0).all())


def test_slots_increase_and_pair_of_slot_inverts(amd, golden):
    for name, c in cases(amd, golden):
        hit = dense64(c)["hit"]
        for cap in (32, RC.capacity(int(hit.sum(0).max())), RC.capacity(c["Nr"]) + 32):
            scan, slot, kept, count = RC.slots(hit, cap)
            assert scan.dtype == torch.int32 and torch.equal(count.long(), hit.sum(0))
            pos = RC.pair_of_slot(slot, kept, cap)
            for b in range(c["Nb"]):
                rows = torch.nonzero(kept[:, b]).flatten()
                n = rows.numel()
                assert n == min(int(count[b]), cap), name
                assert torch.equal(slot[rows, b].long(), torch.arange(n)), name            # ranks in list order: strictly increasing with r
                assert torch.equal(pos[b, :n].long(), rows) and bool((pos[b, n:] == -1).all()), name


def test_overflow_rule(amd):
    """A hit pair with slot >= C is dropped: not kept, depth -1, sigma 0 and white after the gather; count still tells the truth."""
    c = make_case(amd, 1, 300, 64, seed=365)
    o = dense64(c)
    hit, S = o["hit"], c["S"]
    for cap in (32, 96):
        assert int(hit.sum()) > cap
        comp = RC.scene_samples_compact(o, hit, cap, S)
        dropped = hit & ~comp["kept"]
        assert int(comp["kept"].sum()) == cap and int(dropped.sum()) == int(hit.sum()) - cap == int((comp["count"] - cap).clamp_min(0).sum())
        first_dropped = int(torch.nonzero(dropped[:, 0]).flatten()[0])
        assert not bool(dropped[:first_dropped].any()) and not bool(comp["kept"][first_dropped:].any())      # the first C hits in list order stay
        z = comp["z_vals"].view(c["Nr"], 1, S)
        assert bool((z[dropped] == -1).all()) and torch.equal(z[comp["kept"]], o["z_vals"].view(c["Nr"], 1, S)[comp["kept"]])
        sig, rgb = RC.gather_compact(torch.full((cap * S,), 5.0), torch.full((cap * S, 3), 0.25), comp["slot"], comp["kept"], S)
        assert bool((sig.view(c["Nr"], 1, S)[dropped] == 0).all()) and bool((rgb.view(c["Nr"], 1, S, 3)[dropped] == 1).all())
        assert bool((sig.view(c["Nr"], 1, S)[comp["kept"]] == 5).all())
        assert not bool((comp["pair_of_slot"] < 0).any())


def test_scene_capacity(amd):
    assert [amd.ops.scene_capacity(n) for n in (0, 1, 32, 33)] == [32, 32, 32, 64]
    assert all(amd.ops.scene_capacity(n) == RC.capacity(n) for n in range(0, 200))


# ------------------------------------------------------------------------------------------------ C ABI
NEW = ("snr_scene_pair_hits", "snr_scene_samples_compact_fwd", "snr_scene_samples_compact_bwd", "snr_scene_gather_compact_fwd",
       "snr_scene_gather_compact_bwd")


def test_abi_version_and_symbols(amd):
    hdr = open(os.path.join(os.path.dirname(amd.__file__), "..", "include", "supnerf_hip.h")).read()
    assert amd._lib.header_abi_version() >= 18
    lib = amd._lib.lib()
    assert lib.snr_abi_version() == amd._lib.header_abi_version()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in amd._lib.exported_symbols()
        assert getattr(lib, name) is not None


OK, E_ARG, E_WORKSPACE = 0, -1, -3
P_ = C.c_void_p(0x1000)      # never dereferenced on the host: every case below returns before a launch
N_ = C.c_void_p(0)
K4 = (100.0, 100.0, 40.0, 30.0)
#   cam2obj wlh rois pixels K Nr Nb aabb hit stream
HITS_CASES = {
    "empty_all_null": ((N_, N_, N_, N_, *K4, 0, 3, 1, N_, N_), OK),
    "null_hit": ((P_, P_, P_, P_, *K4, 4, 3, 1, N_, N_), E_ARG),
    "null_rois": ((P_, P_, N_, P_, *K4, 4, 3, 1, P_, N_), E_ARG),
    "no_object": ((P_, P_, P_, P_, *K4, 4, 0, 1, P_, N_), E_ARG),
    "negative_pixels": ((P_, P_, P_, P_, *K4, -1, 3, 1, P_, N_), E_ARG),
}
#   cam2obj wlh rois pixels K jitter Nr Nb S scale aabb shapenet scan C | xyz viewdir z kept pair_of_slot stream
FWD_CASES = {
    "no_capacity": ((P_, P_, P_, P_, *K4, N_, 4, 3, 16, 1.0, 1, 1, P_, 0, P_, P_, P_, P_, P_, N_), E_ARG),
    "negative_capacity": ((P_, P_, P_, P_, *K4, N_, 4, 3, 16, 1.0, 1, 1, P_, -32, P_, P_, P_, P_, P_, N_), E_ARG),
    "capacity_33": ((P_, P_, P_, P_, *K4, N_, 4, 3, 16, 1.0, 1, 1, P_, 33, P_, P_, P_, P_, P_, N_), E_ARG),
    "capacity_16": ((P_, P_, P_, P_, *K4, N_, 4, 3, 16, 1.0, 1, 1, P_, 16, P_, P_, P_, P_, P_, N_), E_ARG),
    "empty_bad_capacity": ((N_, N_, N_, N_, *K4, N_, 0, 3, 16, 1.0, 1, 1, N_, 31, N_, N_, N_, N_, N_, N_), E_ARG),
    "null_scan": ((P_, P_, P_, P_, *K4, N_, 4, 3, 16, 1.0, 1, 1, N_, 32, P_, P_, P_, P_, P_, N_), E_ARG),
    "null_pair_of_slot": ((P_, P_, P_, P_, *K4, N_, 4, 3, 16, 1.0, 1, 1, P_, 32, P_, P_, P_, P_, N_, N_), E_ARG),
    "null_kept": ((P_, P_, P_, P_, *K4, N_, 4, 3, 16, 1.0, 1, 1, P_, 32, P_, P_, P_, N_, P_, N_), E_ARG),
    "no_sample": ((P_, P_, P_, P_, *K4, N_, 4, 3, 0, 1.0, 1, 1, P_, 32, P_, P_, P_, P_, P_, N_), E_ARG),
    "too_many_objects": ((P_, P_, P_, P_, *K4, N_, 4, 65536, 16, 1.0, 1, 1, P_, 32, P_, P_, P_, P_, P_, N_), E_ARG),
}
#   ... scan C | d_xyz d_viewdir d_z d_cam2obj ws ws_bytes stream
BWD_CASES = {
    "empty": ((N_, N_, N_, N_, *K4, N_, 0, 3, 16, 1.0, 1, 1, N_, 32, N_, N_, N_, N_, N_, 0, N_), OK),
    "capacity_33": ((P_, P_, P_, P_, *K4, N_, 4, 3, 16, 1.0, 1, 1, P_, 33, P_, P_, P_, P_, P_, 1 << 20, N_), E_ARG),
    "no_capacity": ((P_, P_, P_, P_, *K4, N_, 4, 3, 16, 1.0, 1, 1, P_, 0, P_, P_, P_, P_, P_, 1 << 20, N_), E_ARG),
    "null_scan": ((P_, P_, P_, P_, *K4, N_, 4, 3, 16, 1.0, 1, 1, N_, 32, P_, P_, P_, P_, P_, 1 << 20, N_), E_ARG),
    "null_out": ((P_, P_, P_, P_, *K4, N_, 4, 3, 16, 1.0, 1, 1, P_, 32, P_, P_, P_, N_, P_, 1 << 20, N_), E_ARG),
    "odd_ws": ((P_, P_, P_, P_, *K4, N_, 4, 3, 16, 1.0, 1, 1, P_, 32, P_, P_, P_, P_, C.c_void_p(0x1004), 1 << 20, N_), E_ARG),
    "small_ws": ((P_, P_, P_, P_, *K4, N_, 257, 3, 16, 1.0, 1, 1, P_, 32, P_, P_, P_, P_, P_, 2 * 3 * 12 * 8 - 1, N_), E_WORKSPACE),
}
#   in_sig in_rgb scan kept Nr Nb S C out_sig out_rgb stream
GATHER_FWD_CASES = {
    "empty": ((N_, N_, N_, N_, 0, 3, 16, 32, N_, N_, N_), OK),
    "capacity_48": ((P_, P_, P_, P_, 4, 3, 16, 48, P_, P_, N_), E_ARG),
    "no_capacity": ((P_, P_, P_, P_, 4, 3, 16, 0, P_, P_, N_), E_ARG),
    "null_scan": ((P_, P_, N_, P_, 4, 3, 16, 32, P_, P_, N_), E_ARG),
    "null_kept": ((P_, P_, P_, N_, 4, 3, 16, 32, P_, P_, N_), E_ARG),
    "no_output": ((P_, P_, P_, P_, 4, 3, 16, 32, N_, N_, N_), E_ARG),
    "output_without_input": ((N_, P_, P_, P_, 4, 3, 16, 32, P_, P_, N_), E_ARG),
}
#   d_sig_rows d_rgb_rows pair_of_slot Nr Nb S C d_sig d_rgb stream
GATHER_BWD_CASES = {
    "capacity_48": ((P_, P_, P_, 4, 3, 16, 48, P_, P_, N_), E_ARG),
    "no_capacity": ((P_, P_, P_, 4, 3, 16, 0, P_, P_, N_), E_ARG),
    "null_pair_of_slot": ((P_, P_, N_, 4, 3, 16, 32, P_, P_, N_), E_ARG),
    "no_output": ((P_, P_, P_, 4, 3, 16, 32, N_, N_, N_), E_ARG),
    "output_without_input": ((N_, P_, P_, 4, 3, 16, 32, P_, P_, N_), E_ARG),
    "no_sample": ((P_, P_, P_, 4, 3, 0, 32, P_, P_, N_), E_ARG),
}
ABI_CASES = {"snr_scene_pair_hits": HITS_CASES, "snr_scene_samples_compact_fwd": FWD_CASES, "snr_scene_samples_compact_bwd": BWD_CASES,
             "snr_scene_gather_compact_fwd": GATHER_FWD_CASES, "snr_scene_gather_compact_bwd": GATHER_BWD_CASES}


@pytest.mark.parametrize("fn,name", [(f, n) for f, t in ABI_CASES.items() for n in t])
def test_argument_checks(amd, fn, name):
    args, want = ABI_CASES[fn][name]
    assert getattr(amd._lib.lib(), fn)(*args) == want


# ------------------------------------------------------------------------------------------------ operators
def test_operator_errors(amd):
    ops = amd.ops
    cam2obj, wlh = torch.eye(3, 4)[None].repeat(2, 1, 1), torch.ones(2, 3)
    rois = torch.tensor([[0, 0, 8, 8], [0, 0, 8, 8]], dtype=torch.int32)
    pixels = torch.tensor([[1, 1], [2, 3]], dtype=torch.int32)
    Kvec = (10.0, 10.0, 4.0, 4.0)
    with pytest.raises(amd.SnrError, match="GPU"):
        ops.scene_pair_hits(cam2obj, wlh, rois, pixels, Kvec)
    for args in ((cam2obj[:, :, :3], wlh, rois, pixels, Kvec), (cam2obj, wlh[:1], rois, pixels, Kvec), (cam2obj, wlh, rois.long(), pixels, Kvec),
                 (cam2obj, wlh, rois, pixels.long(), Kvec), (cam2obj, wlh, rois, pixels[:, :1], Kvec), (cam2obj, wlh, rois, pixels, Kvec[:3])):
        with pytest.raises(amd.SnrError, match="scene_pair_hits"):
            ops.scene_pair_hits(*args)

    scan = torch.ones(2, 2, dtype=torch.int32)
    good = (cam2obj, wlh, rois, pixels, Kvec, None, 4, 1.0, True, True, scan, 32)
    with pytest.raises(amd.SnrError, match="GPU"):
        ops.SceneSamplesCompact.apply(*good)

    def bad(i, v):
        a = list(good)
        a[i] = v
        with pytest.raises(amd.SnrError, match="scene_samples_compact"):
            ops.SceneSamplesCompact.apply(*a)
    bad(0, cam2obj[:, :, :3]); bad(1, wlh[:1]); bad(2, rois.long()); bad(3, pixels[:, :1]); bad(5, torch.zeros(3, 4)); bad(6, 0); bad(4, (1.0, 1.0, 1.0))
    bad(10, scan.long()); bad(10, scan[:1]); bad(10, scan.t()[:, :1]); bad(11, 0); bad(11, 33); bad(11, -32); bad(11, 32.0); bad(11, None)

    kept, pos = torch.ones(2, 2, dtype=torch.uint8), torch.zeros(2, 32, dtype=torch.int32)
    n = 2 * 32 * 4
    with pytest.raises(amd.SnrError, match="GPU"):
        ops.SceneGatherCompact.apply(torch.zeros(n), torch.zeros(n, 3), scan, kept, pos, 4)
    for args in ((torch.zeros(n - 1), torch.zeros(n, 3), scan, kept, pos, 4), (torch.zeros(n), torch.zeros(n, 2), scan, kept, pos, 4),
                 (torch.zeros(n), torch.zeros(n, 3), scan, kept.bool(), pos, 4), (torch.zeros(n), torch.zeros(n, 3), scan, kept, pos.long(), 4),
                 (torch.zeros(n), torch.zeros(n, 3), scan.long(), kept, pos, 4), (torch.zeros(n), torch.zeros(n, 3), scan[:1], kept, pos, 4),
                 (torch.zeros(n), torch.zeros(n, 3), scan, kept, pos, 0), (torch.zeros(n), torch.zeros(n, 3), scan, kept, pos[:1], 4),
                 (torch.zeros(2 * 48 * 4), torch.zeros(2 * 48 * 4, 3), scan, kept, torch.zeros(2, 48, dtype=torch.int32), 4)):
        with pytest.raises(amd.SnrError, match="scene_gather_compact"):
            ops.SceneGatherCompact.apply(*args)


def test_render_scene_misuse(amd, golden):
    g = golden("scene")
    H, W = int(g["H"]), int(g["W"])
    pixels = torch.tensor([[10, 10], [11, 10]])
    args = (g["obj_poses"], g["obj_wlh"], g["shapecodes"], g["texturecodes"], g["K"], pixels, H, W, 4)
    foreign = torch.nn.Linear(1, 1)
    with pytest.raises(amd.SnrError, match="fused"):
        amd.scene.render_scene(foreign, "cpu", *args, compact=True)
    with pytest.raises(amd.SnrError, match="fused"):
        amd.scene.render_scene(foreign, "cpu", *args, compact=True, capacity=32)
    with pytest.raises(amd.SnrError, match="decoder"):
        amd.scene.render_scene(foreign, "cpu", *args, fused=True, compact=True)
    with pytest.raises(amd.SnrError, match="compact"):
        amd.scene.render_scene(foreign, "cpu", *args, fused=True, capacity=32)
