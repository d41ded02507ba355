"""CPU tests of the differentiable scene render: the dense restatement of the merge + composite (tests/scene_grad_restatement.py) against
``oracle.scene_composite`` in values and in autograd, its rule on tied depths, ``scene.scene_ray_rows`` against ``scene.scene_rays`` and
under gradcheck, and the argument checks of snr_scene_composite_bwd (no launch is made)."""
import ctypes as C

import pytest
import torch

import scene_grad_restatement as R
from oracle import supnerf_oracle as O
from oracle_bands import amd, in_band  # noqa: F401  (amd: a fixture)

SHAPES = [(1, 64, 37), (3, 64, 101), (4, 64, 57), (2, 128, 40), (4, 32, 77), (8, 32, 33), (7, 33, 50), (2, 5, 300), (8, 64, 20)]


@pytest.mark.parametrize("quarters", [False, True])
@pytest.mark.parametrize("Nb,S,P", SHAPES)
def test_restatement_equals_oracle(Nb, S, P, quarters):
    """Forward: exactly ``oracle.scene_composite`` in float64, ties or not.  Autograd: exactly the oracle's on every pixel without a tie
    between real samples (on tied pixels torch's scatter_ / sort backward is arbitrary; the restatement's rule is tested below)."""
    sig, rgb, z = [t.double() for t in R.shape_case(Nb, S, P, quarters)]
    gen = torch.Generator().manual_seed(P)
    w = [torch.randn(P, 3, generator=gen).double(), torch.randn(P, generator=gen).double(), torch.randn(P, generator=gen).double()]
    res = []
    for fn in (R.scene_composite, O.scene_composite):
        a, b, c = [t.clone().requires_grad_() for t in (sig, rgb, z)]
        out = fn(a, b, c)
        g = torch.autograd.grad(sum((o * wi).sum() for o, wi in zip(out, w)), (a, b, c))
        res.append((out, g))
    for mine, theirs in zip(res[0][0], res[1][0]):
        assert torch.equal(mine, theirs)
    free = R.tie_free(z)
    if quarters:
        assert not bool(free.all())           # the rounded variant is there for its ties
    else:
        assert bool(free.any())
    for mine, theirs in zip(res[0][1], res[1][1]):
        assert torch.equal(mine[free], theirs[free])


def test_tied_groups_by_hand():
    """One pixel, 2 objects x 3 samples, written out.  Memory order: object 0 = (2, 3, 3), object 1 = (3, 4, 4).
    Depth 3 is shared by samples 1, 2, 3: lt = 1, slots 1, 2, 3 in memory order, survivor sample 3 feeds slot 1 (interval 3 -> 3: width 0).
    Depth 4 by samples 4, 5: lt = 4, slots 4, 5, survivor sample 5 feeds slot 4 (width 0).  Sample 0 (depth 2) is alone in slot 0.
    Sorted rows: z = (2, 3, 3, 3, 4, 4), sigma = (s0, s3, 0, 0, s5, 0)."""
    z = torch.tensor([[2.0, 3.0, 3.0, 3.0, 4.0, 4.0]], dtype=torch.float64)
    sig = torch.tensor([[0.7, 0.9, 1.1, 1.3, 0.5, 0.8]], dtype=torch.float64)
    rgb = torch.linspace(0.1, 0.9, 18, dtype=torch.float64).view(1, 6, 3)
    lt, eb, ea = R.ranks(z)
    assert lt.tolist() == [[0, 1, 1, 1, 4, 4]] and eb.tolist() == [[0, 0, 1, 2, 0, 1]] and ea.tolist() == [[0, 2, 1, 0, 1, 0]]
    s_sort, c_sort, z_sort = R.merged_rows(sig, rgb, z)
    assert z_sort.tolist() == [[2.0, 3.0, 3.0, 3.0, 4.0, 4.0]]
    assert s_sort.tolist() == [[0.7, 1.3, 0.0, 0.0, 0.8, 0.0]]
    assert torch.equal(c_sort[0, 1], rgb[0, 3]) and torch.equal(c_sort[0, 4], rgb[0, 5]) and float(c_sort[0, [2, 3, 5]].abs().max()) == 0
    w_rgb, w_d, w_a = torch.tensor([[0.3, -1.1, 0.6]], dtype=torch.float64), torch.tensor([0.8], dtype=torch.float64), torch.tensor([-0.4], dtype=torch.float64)
    d_sig, d_rgb, d_z = R.grads(sig, rgb, z, w_rgb, w_d, w_a)
    # every member of a tied group: zero d_sigma and d_rgb -- the dropped ones by the rule, the survivors because their interval has width 0.
    # (Sample 5 survives INTO slot 4, width 4 -> 4; the LAST_DELTA interval belongs to slot 5, which holds sigma 0.)
    assert float(d_sig[0, 1:].abs().max()) == 0 and float(d_rgb[0, 1:].abs().max()) == 0
    assert float(d_sig[0, 0].abs()) > 0 and float(d_rgb[0, 0].abs().min()) > 0
    # d_z follows the slots: composite backward on the sorted rows, slot k -> the sample that owns slot k (here the identity permutation)
    a, b, c = [t.clone().requires_grad_() for t in (s_sort, c_sort, z_sort)]
    out = O.composite(a, b, c, True)
    want = torch.autograd.grad((out[0] * w_rgb).sum() + (out[1] * w_d).sum() + (out[2] * w_a).sum(), c)[0]
    assert torch.equal(d_z, want)
    # a zero-width interval still has a slope in its width, so the tied slots carry d_z: slot k gets dd_{k-1} - dd_k with dd_k the gradient of
    # interval k's width; slot 3 sits between two zero-density slots (dd_2 = dd_3 = 0)
    assert float(d_z[0, [0, 1, 2, 4, 5]].abs().min()) > 0 and float(d_z[0, 3]) == 0
    # the same pixel with the objects swapped in memory, (3, 4, 4, 2, 3, 3): the slots follow memory order again.  Depth 3 = samples 0, 4, 5
    # -> slots 1, 2, 3, survivor sample 5; depth 4 = samples 1, 2 -> slots 4, 5, survivor sample 2; depth 2 = sample 3 -> slot 0
    perm = torch.tensor([3, 4, 5, 0, 1, 2])
    sig2, rgb2, z2 = sig[:, perm], rgb[:, perm], z[:, perm]
    lt2, eb2, ea2 = R.ranks(z2)
    assert (lt2 + eb2).tolist() == [[1, 4, 5, 0, 2, 3]] and (ea2 == 0).tolist() == [[False, False, True, True, False, True]]
    d_sig2, d_rgb2, d_z2 = R.grads(sig2, rgb2, z2, w_rgb, w_d, w_a)
    a, b, c = [t.clone().requires_grad_() for t in R.merged_rows(sig2, rgb2, z2)]
    assert a.tolist() == [[0.7, 1.1, 0.0, 0.0, 0.8, 0.0]]
    out = O.composite(a, b, c, True)
    want2 = torch.autograd.grad((out[0] * w_rgb).sum() + (out[1] * w_d).sum() + (out[2] * w_a).sum(), c)[0]
    assert torch.equal(d_z2, want2[:, [1, 4, 5, 0, 2, 3]])
    assert float(d_sig2[0, [0, 1, 2, 4, 5]].abs().max()) == 0 and float(d_sig2[0, 3].abs()) > 0


# ------------------------------------------------------------------------------------------------ scene_ray_rows
@pytest.fixture(scope="module")
def scene(golden):
    g = golden("scene")
    H, W = int(g["H"]), int(g["W"])
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return g, H, W, torch.stack([xs.reshape(-1), ys.reshape(-1)], 1)          # every pixel, row-major like the table


@pytest.mark.parametrize("rend_aabb", [True, False])
def test_scene_ray_rows_match_scene_rays(amd, scene, rend_aabb):
    g, H, W, pixels = scene
    S = amd.scene
    table, valid, _ = S.scene_rays(g["obj_poses"], g["obj_wlh"], g["K"], H, W, rend_aabb=rend_aabb)
    table = table.view(H * W, -1, 8)
    got, got_valid = S.scene_ray_rows(g["obj_poses"], g["obj_wlh"], g["K"], pixels, H, W, rend_aabb=rend_aabb)
    o64, _ = S.scene_ray_rows(g["obj_poses"].double(), g["obj_wlh"], g["K"], pixels, H, W, rend_aabb=rend_aabb)
    assert got.dtype == torch.float32 and got.shape == table.shape and o64.dtype == torch.float64
    hits = (o64[..., 7] - o64[..., 6]) > 0                                    # (pixel, object) pairs that meet their box, in float64
    in_roi = ~(o64 == -1.0).all(-1)
    if rend_aabb:
        # the float64 slab gap |far - near| of every in-roi pair, hit or miss: a thin one is a grazing ray that fp32 may call either way
        diag = g["obj_wlh"].double().norm(dim=1)
        half = (g["obj_wlh"].double()[:, [1, 0, 2]] / diag[:, None])[None].expand(H * W, -1, -1)
        t_near, t_far, _ = amd.utils._slab(o64[..., :3], o64[..., 3:6], -half, half)
        gap = (t_far - t_near).abs()
        thin = in_roi & (gap < 1e-3)
        print(f"hits {int(hits.sum())}; thinner than 1e-3: {int((thin & hits).sum())} hits, {int((thin & ~hits).sum())} misses; "
              f"thinner than 1e-2: {int((hits & (gap < 1e-2)).sum())} hits, {int((in_roi & ~hits & (gap < 1e-2)).sum())} misses")
        assert int(hits.sum()) == 1627 and int((thin & hits).sum()) == 0 and int((hits & (gap < 1e-2)).sum()) == 3
    else:
        thin = torch.zeros_like(hits)                                         # sphere bounds: no slab test, nothing grazes
    assert int(thin.sum()) <= 0.01 * int(in_roi.sum())
    keep = ~thin
    minus = lambda t: t == -1.0                                               # noqa: E731
    assert torch.equal(minus(got)[keep], minus(table)[keep]) and torch.equal(minus(got)[keep], minus(o64)[keep])
    keep_px = keep.all(1)
    assert torch.equal(got_valid[keep_px], valid[keep_px])
    ok, _, msg = in_band(got[keep], table[keep], o64[keep], "fp32", "scene_ray_rows")
    print(msg)
    assert ok, msg


@pytest.mark.parametrize("rend_aabb", [True, False])
def test_scene_ray_rows_gradcheck(amd, scene, rend_aabb):
    g, H, W, pixels = scene
    S = amd.scene
    rows, _ = S.scene_ray_rows(g["obj_poses"].double(), g["obj_wlh"], g["K"], pixels, H, W)
    all3 = torch.nonzero(((rows[..., 7] - rows[..., 6]) > 0).all(1)).flatten()
    assert all3.numel() == 150
    px = pixels[all3[torch.linspace(0, 149, 8).long()]]
    poses = g["obj_poses"].double().clone().requires_grad_()
    assert torch.autograd.gradcheck(lambda p: S.scene_ray_rows(p, g["obj_wlh"], g["K"], px, H, W, rend_aabb=rend_aabb)[0], (poses,))


# ------------------------------------------------------------------------------------------------ C ABI
OK, E_ARG, E_SHAPE, E_UNSUPPORTED = 0, -1, -2, -5
P_ = C.c_void_p(0x1000)      # never dereferenced on the host: every case below returns before a launch
N_ = C.c_void_p(0)
#                sigmas rgbs z   P  n   run flags d_rgb d_depth d_acc d_sig d_rgbs d_z stream
ABI_CASES = {
    "empty_all_null": ((N_, N_, N_, 0, 64, 0, 1, N_, N_, N_, N_, N_, N_, N_), OK),
    "empty_bad_n": ((N_, N_, N_, 0, 513, 7, 1, N_, N_, N_, N_, N_, N_, N_), OK),
    "null_sigmas": ((N_, P_, P_, 4, 64, 0, 1, P_, N_, N_, P_, P_, N_, N_), E_ARG),
    "null_rgbs": ((P_, N_, P_, 4, 64, 0, 1, P_, N_, N_, P_, P_, N_, N_), E_ARG),
    "null_z": ((P_, P_, N_, 4, 64, 0, 1, P_, N_, N_, P_, P_, N_, N_), E_ARG),
    "null_d_rgb": ((P_, P_, P_, 4, 64, 0, 1, N_, P_, P_, P_, P_, P_, N_), E_ARG),
    "null_d_sigmas": ((P_, P_, P_, 4, 64, 0, 1, P_, N_, N_, N_, P_, N_, N_), E_ARG),
    "null_d_rgbs": ((P_, P_, P_, 4, 64, 0, 1, P_, N_, N_, P_, N_, N_, N_), E_ARG),
    "negative_pixels": ((P_, P_, P_, -1, 64, 0, 1, P_, N_, N_, P_, P_, N_, N_), E_ARG),
    "n_0": ((P_, P_, P_, 4, 0, 0, 1, P_, N_, N_, P_, P_, N_, N_), E_ARG),
    "negative_run": ((P_, P_, P_, 4, 64, -1, 1, P_, N_, N_, P_, P_, N_, N_), E_ARG),
    "run_not_dividing": ((P_, P_, P_, 4, 64, 48, 1, P_, N_, N_, P_, P_, N_, N_), E_SHAPE),
    "null_before_shape": ((N_, P_, P_, 4, 64, 48, 1, P_, N_, N_, P_, P_, N_, N_), E_ARG),
    "n_513": ((P_, P_, P_, 4, 513, 0, 1, P_, N_, N_, P_, P_, P_, N_), E_UNSUPPORTED),
    "n_1026_run_513": ((P_, P_, P_, 4, 1026, 513, 1, P_, N_, N_, P_, P_, P_, N_), E_UNSUPPORTED),
    "shape_before_limit": ((P_, P_, P_, 4, 513, 64, 1, P_, N_, N_, P_, P_, P_, N_), E_SHAPE),
}


def test_abi_version_and_symbol(amd):
    assert amd._lib.header_abi_version() >= 16
    assert "snr_scene_composite_bwd" in amd._lib.exported_symbols()
    assert amd._lib.lib().snr_abi_version() == amd._lib.header_abi_version()


@pytest.mark.parametrize("name", list(ABI_CASES))
def test_scene_composite_bwd_argument_checks(amd, name):
    args, want = ABI_CASES[name]
    assert amd._lib.lib().snr_scene_composite_bwd(*args) == want
