"""GPU tests of the compact scene route: snr_scene_pair_hits, snr_scene_samples_compact_fwd / bwd and snr_scene_gather_compact_fwd / bwd behind
``ops.scene_pair_hits`` / ``ops.SceneSamplesCompact`` / ``ops.SceneGatherCompact``, ``scene.render_pairs(capacity=...)``,
``scene.render_scene(compact=True)`` and ``driver.optimize_scene(compact=True)``.

The yardsticks are the dense kernels (``ops.SceneSamples`` / ``ops.SceneGather``, unchanged by this route) and the copies and fills of
tests/scene_compact_restatement.py applied to THEIR outputs; hit counts come from the dense kernel's own ``hit``.  Everything up to the
decoder is compared bit for bit (int32 views of the fp32 tensors).  The decoder's latent-gradient sum runs over other tiles on the compact
route, so ``render_scene`` and ``optimize_scene`` are held to the bands tests/test_scene_rows_gpu.py and tests/test_scene_fit_gpu.py build
from the existing routes: 4 x the distance between the default route with fp32 and with float64 pose leaves, floor one fp32 ulp."""
import warnings

import numpy as np
import pytest
import torch

import scene_compact_restatement as RC
import scene_rows_restatement as R
from oracle_bands import amd, dev, make_model  # noqa: F401  (amd, dev: fixtures)
from test_scene_fit_gpu import NOISE, SEED, T, setup, twin  # noqa: F401  (setup: a fixture)
from test_scene_rows_gpu import BWD_CASES, SHAPES, kernel, make_case, render_with_grads, scene, ulp_of  # noqa: F401  (scene: a fixture)

pytestmark = pytest.mark.gpu

VARIANTS = dict(sphere=dict(rend_aabb=False), object_frame=dict(shapenet=False), scaled=dict(scale=0.6), no_jitter=dict(jitter=False))


def bits(a, b):
    """The same shape, dtype and bits (-0.0 is not 0.0, NaN payloads count)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return torch.equal(a, b)


def trimmed(c, n):
    """The case with its first n pixels."""
    d = dict(c)
    d["pixels"], d["Nr"] = c["pixels"][:n], n
    d["jitter"] = None if c["jitter"] is None else c["jitter"][:n * c["Nb"]]
    return d


def run_compact(amd, dev, c, cap, scan, cam2obj=None):
    cam2obj = R.cam2obj_of(c["poses"]).to(dev) if cam2obj is None else cam2obj
    jit = c["jitter"]
    return amd.ops.SceneSamplesCompact.apply(cam2obj, c["wlh"].to(dev), c["rois"].to(dev), c["pixels"].to(dev), c["Kvec"],
                                             None if jit is None else jit.to(dev), c["S"], c["scale"], c["rend_aabb"], c["shapenet"], scan, cap)


def check_compact(amd, dev, c, cap, name, full=False):
    """The compact forward with capacity ``cap`` against the dense forward of the same case, compacted by the restatement; -> (dense hit,
    what the restatement made)."""
    d = kernel(amd, dev, c)
    hit = d[3]
    want = RC.scene_samples_compact(d, hit, cap, c["S"])
    got = run_compact(amd, dev, c, cap, want["scan"])
    assert len(got) == 5
    for k, g in zip(("xyz", "viewdir", "z_vals"), got):
        assert bits(g, want[k]), (name, cap, k)
    assert got[3].dtype == torch.uint8 and torch.equal(got[3].bool(), want["kept"]), (name, cap)
    assert got[4].dtype == torch.int32 and torch.equal(got[4], want["pair_of_slot"]), (name, cap)
    count = hit.sum(0)
    if full:       # nothing dropped: the dense flags and the dense depths as they are
        assert int(count.max()) <= cap and torch.equal(got[3], hit) and bits(got[2], d[2]), (name, cap)
    # the stated constants on padding, whoever wrote them
    pad = (got[4] < 0).reshape(-1)
    assert int(pad.sum()) == int((cap - count.clamp(max=cap)).sum())
    assert bool((got[0][pad] == 0).all()) and bits(got[1][pad], torch.tensor([0.0, 0.0, 1.0], device=dev).expand(int(pad.sum()), c["S"], 3).contiguous())
    return hit, want


# ------------------------------------------------------------------------------------------------ 1. the flags alone
@pytest.mark.parametrize("Nb,Nr,S", SHAPES)
def test_pair_hits_are_the_dense_flags(amd, dev, Nb, Nr, S):
    for kw in ({}, dict(rend_aabb=False)):
        c = make_case(amd, Nb, Nr, S, seed=Nb + Nr + S, **kw)
        hit = amd.ops.scene_pair_hits(R.cam2obj_of(c["poses"]).to(dev), c["wlh"].to(dev), c["rois"].to(dev), c["pixels"].to(dev), c["Kvec"], c["rend_aabb"])
        want = kernel(amd, dev, c)[3]
        assert hit.dtype == torch.uint8 and hit.shape == (Nr, Nb) and torch.equal(hit, want)
        assert bool(((hit == 0) | (hit == 1)).all())


# ------------------------------------------------------------------------------------------------ 2. forward, nothing dropped
@pytest.mark.parametrize("Nb,Nr,S", SHAPES)
def test_forward_is_the_dense_forward(amd, dev, Nb, Nr, S):
    c = make_case(amd, Nb, Nr, S, seed=Nb + Nr + S)
    count = kernel(amd, dev, c)[3].sum(0)
    check_compact(amd, dev, c, amd.ops.scene_capacity(int(count.max())), f"({Nb},{Nr},{S})", full=True)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_forward_variants(amd, dev, variant):
    c = make_case(amd, 3, 300, 16, seed=5, **VARIANTS[variant])
    count = kernel(amd, dev, c)[3].sum(0)
    assert int(count.max()) > 0
    check_compact(amd, dev, c, amd.ops.scene_capacity(int(count.max())), variant, full=True)


# ------------------------------------------------------------------------------------------------ 3. capacity edges
EDGES = [(1, 300, 64), (8, 1025, 2), (3, 257, 1)]


def gather_of_dropped(amd, dev, c, cap, hit, want):
    """After the gather a dropped pair is (0, white), like one that is not hit; kept pairs take their slot's rows."""
    S, Nr, Nb = c["S"], c["Nr"], c["Nb"]
    gen = torch.Generator().manual_seed(cap)
    sig, rgb = torch.randn(Nb * cap * S, generator=gen).to(dev), torch.rand(Nb * cap * S, 3, generator=gen).to(dev)
    got = amd.ops.SceneGatherCompact.apply(sig, rgb, want["scan"], want["kept"].to(torch.uint8), want["pair_of_slot"], S)
    ref = RC.gather_compact(sig, rgb, want["slot"], want["kept"], S)
    assert bits(got[0], ref[0]) and bits(got[1], ref[1])
    dropped = hit.bool() & ~want["kept"]
    assert bool((got[0].view(Nr, Nb, S)[dropped] == 0).all()) and bool((got[1].view(Nr, Nb, S, 3)[dropped] == 1).all())
    return dropped


@pytest.mark.parametrize("Nb,Nr,S", EDGES)
def test_capacity_edges(amd, dev, Nb, Nr, S):
    c = make_case(amd, Nb, Nr, S, seed=Nb + Nr + S)
    hit = kernel(amd, dev, c)[3]
    count = hit.sum(0)
    top = int(count.max())
    if (Nb, Nr, S) == (1, 300, 64):
        assert top == 192 and int(hit[:256].sum()) == 163
    if (Nb, Nr, S) == (8, 1025, 2):
        assert int(count.min()) == 21 and top == 151
    if (Nb, Nr, S) == (3, 257, 1):
        assert not bool(hit[256:].any())                                                         # the one-pixel last slice is empty
    # an exact fit: the list trimmed where the dense scan of the then fullest object reaches a multiple of 32 (the longest such list)
    scan = torch.cumsum(hit.to(torch.int32), 0, dtype=torch.int32).cpu()
    fits = [(int(r) + 1, int(scan[r, b])) for b in range(Nb) for r in torch.nonzero(hit[:, b].cpu()).flatten()
            if int(scan[r, b]) % 32 == 0 and int(scan[r].max()) == int(scan[r, b])]
    assert fits, "no object of this case ever fills a whole number of 32-slot tiles as the fullest one"
    fit = max(fits)
    _, want = check_compact(amd, dev, trimmed(c, fit[0]), fit[1], f"fit {fit}", full=True)
    assert int((want["pair_of_slot"] >= 0).all(1).sum()) >= 1                                    # some object has no padding slot at all
    # a capacity above every count: padding on every object
    _, want = check_compact(amd, dev, c, amd.ops.scene_capacity(top) + 32, "roomy", full=True)
    assert bool((want["pair_of_slot"][:, -32:] == -1).all())
    # capacities below the count: the drop lands inside slice 0 and in later slices
    first = []
    for cap in (32, 96):
        if top <= cap:
            continue
        _, want = check_compact(amd, dev, c, cap, "short")
        dropped = gather_of_dropped(amd, dev, c, cap, hit, want)
        assert int(dropped.sum()) == int((count - cap).clamp(min=0).sum()) > 0
        z = want["z_vals"].view(Nr, Nb, S)
        assert bool((z[dropped] == -1).all())
        first += [int(torch.nonzero(dropped[:, b]).flatten()[0]) // 256 for b in range(Nb) if bool(dropped[:, b].any())]
    print(f"({Nb},{Nr},{S}): counts {count.tolist()}, exact fit {fit}, first dropped pair in slices {first}")
    if (Nb, Nr, S) == (1, 300, 64):
        assert first == [0, 0]
    if (Nb, Nr, S) == (8, 1025, 2):
        assert len(first) >= 8 and min(first) >= 0 and max(first) >= 1 and len(set(first)) >= 2


def test_dead_roi_is_all_padding(amd, dev):
    c = make_case(amd, 3, 300, 16, seed=5)
    c["rois"] = c["rois"].clone()
    c["rois"][1] = torch.tensor([40, 10, 40, 30], dtype=torch.int32)
    count = kernel(amd, dev, c)[3].sum(0)
    assert int(count[1]) == 0 and int(count[0]) > 0 and int(count[2]) > 0
    cap = amd.ops.scene_capacity(int(count.max()))
    _, want = check_compact(amd, dev, c, cap, "dead roi", full=True)
    assert bool((want["pair_of_slot"][1] == -1).all()) and not bool(want["kept"][:, 1].any())


def test_no_pixel_is_padding_only(amd, dev):
    c = trimmed(make_case(amd, 3, 16, 5, seed=2), 0)
    scan = torch.zeros(0, 3, dtype=torch.int32, device=dev)
    cam2obj = R.cam2obj_of(c["poses"]).to(dev).requires_grad_()
    xyz, viewdir, z, kept, pos = run_compact(amd, dev, c, 64, scan, cam2obj)
    assert xyz.shape == (3 * 64, 5, 3) and z.shape == (0, 15) and kept.shape == (0, 3) and pos.shape == (3, 64)
    assert bool((xyz == 0).all()) and bool((pos == -1).all())
    assert bits(viewdir, torch.tensor([0.0, 0.0, 1.0], device=dev).expand(3 * 64, 5, 3).contiguous())
    g, = torch.autograd.grad((xyz,), cam2obj, (torch.ones_like(xyz),))
    assert bool((g == 0).all())
    hit = amd.ops.scene_pair_hits(cam2obj, c["wlh"].to(dev), c["rois"].to(dev), c["pixels"].to(dev), c["Kvec"])
    assert hit.shape == (0, 3)


# ------------------------------------------------------------------------------------------------ 4. gather
@pytest.mark.parametrize("Nb,Nr,S,short", [(1, 1, 1, False), (3, 65, 16, False), (8, 300, 65, False), (3, 1025, 2, False), (3, 300, 4, True)])
def test_gather_is_the_dense_gather(amd, dev, Nb, Nr, S, short):
    """Scattered random inputs: the compact gather of compact rows == the dense gather of the same rows scattered to the dense layout (there
    with ``hit`` = the kept pairs), forward and backward, bit for bit; padding gradients exactly 0; each input alone."""
    ops = amd.ops
    gen = torch.Generator().manual_seed(Nr)
    hit = (torch.rand(Nr, Nb, generator=gen) < 0.5).to(torch.uint8).to(dev)
    hit[0, 0] = 1
    top = int(hit.sum(0).max())
    cap = 32 if short else ops.scene_capacity(top)
    assert (top > cap) == short
    scan, slot, kept, _ = RC.slots(hit, cap)
    pos = RC.pair_of_slot(slot, kept, cap)
    sig_c, rgb_c = torch.randn(Nb * cap * S, generator=gen).to(dev), torch.rand(Nb * cap * S, 3, generator=gen).to(dev)
    sig_d = RC.scatter_rows(sig_c.view(-1, S), slot, kept, float("nan")).reshape(-1)              # (what a miss holds is never read)
    rgb_d = RC.scatter_rows(rgb_c.view(-1, S, 3), slot, kept, float("nan")).reshape(-1, 3)
    ws, wr = torch.randn(Nr, Nb * S, generator=gen).to(dev), torch.randn(Nr, Nb * S, 3, generator=gen).to(dev)
    kept8 = kept.to(torch.uint8)
    a, b = sig_c.clone().requires_grad_(), rgb_c.clone().requires_grad_()
    a_d, b_d = sig_d.clone().requires_grad_(), rgb_d.clone().requires_grad_()
    got, want = ops.SceneGatherCompact.apply(a, b, scan, kept8, pos, S), ops.SceneGather.apply(a_d, b_d, kept8, S)
    assert bits(got[0], want[0]) and bits(got[1], want[1])
    pad = (pos < 0).reshape(-1)
    for use in ((True, True), (True, False), (False, True)):
        outs = [o for o, u in zip(got, use) if u]
        gs = [w for w, u in zip((ws, wr), use) if u]
        ga = torch.autograd.grad(outs, [t for t, u in zip((a, b), use) if u], gs, retain_graph=True)
        gd = torch.autograd.grad([o for o, u in zip(want, use) if u], [t for t, u in zip((a_d, b_d), use) if u], gs, retain_graph=True)
        for g, d, shape in zip(ga, gd, [s for s, u in zip(((-1, S), (-1, S, 3)), use) if u]):
            assert bits(g.view(shape), RC.compact_rows(d.view(shape), slot, kept, cap, 0.0)), use
            assert bits(g.view(shape)[pad], torch.zeros_like(g.view(shape)[pad])), use          # +0.0 exactly
    ref = RC.gather_compact_bwd(ws, wr, pos, S)
    ga = torch.autograd.grad(got, (a, b), (ws, wr))
    assert bits(ga[0], ref[0]) and bits(ga[1], ref[1])
    # the decoder's (N,S,1) / (N,S,3) shapes pass as they are
    o = ops.SceneGatherCompact.apply(sig_c.view(Nb * cap, S, 1), rgb_c.view(Nb * cap, S, 3), scan, kept8, pos, S)
    assert bits(o[0], got[0]) and bits(o[1], got[1])


# ------------------------------------------------------------------------------------------------ 5. backward to the poses
def upstream(c, cap, pos, seed, dev):
    """Compact upstream gradients, NaN in the rows of padding slots (never read); the depths' dense."""
    gen = torch.Generator().manual_seed(seed)
    Nb, Nr, S = c["Nb"], c["Nr"], c["S"]
    wx, wv = torch.randn(Nb * cap, S, 3, generator=gen).to(dev), torch.randn(Nb * cap, S, 3, generator=gen).to(dev)
    wz = torch.randn(Nr, Nb * S, generator=gen).to(dev)
    pad = (pos < 0).reshape(-1)
    wx[pad] = float("nan")
    wv[pad] = float("nan")
    return wx, wv, wz


def grads_of(outs, leaf, ws, use):
    return torch.autograd.grad([o for o, u in zip(outs, use) if u], leaf, [w for w, u in zip(ws, use) if u], retain_graph=True)[0]


@pytest.mark.parametrize("Nb,Nr,S,variant", BWD_CASES)
def test_backward_is_the_dense_backward(amd, dev, Nb, Nr, S, variant):
    kw = dict(box={}, sphere=dict(rend_aabb=False), object_frame_scaled=dict(shapenet=False, scale=0.6))[variant]
    c = make_case(amd, Nb, Nr, S, seed=3 * Nb + Nr + S, **kw)
    leaf_d = R.cam2obj_of(c["poses"]).to(dev).requires_grad_()
    dense = kernel(amd, dev, c, leaf_d)
    hit = dense[3]
    top = int(hit.sum(0).max())
    caps = [amd.ops.scene_capacity(top)] + ([32] if top > 32 and Nr >= 300 else [])              # the second: pairs are dropped
    for cap in caps:
        scan, slot, kept, _ = RC.slots(hit, cap)
        pos = RC.pair_of_slot(slot, kept, cap)
        leaf = R.cam2obj_of(c["poses"]).to(dev).requires_grad_()
        comp = run_compact(amd, dev, c, cap, scan, leaf)
        assert torch.equal(comp[4], pos)
        wx, wv, wz = upstream(c, cap, pos, Nr + cap, dev)
        # the dense upstream: the compact one scattered; exact zeros on every pair that is not kept (the dense kernel reads them on dropped pairs)
        m1 = kept[:, :, None].expand(Nr, Nb, S).reshape(Nr, Nb * S)
        w_d = (RC.scatter_rows(wx, slot, kept, 0.0), RC.scatter_rows(wv, slot, kept, 0.0), torch.where(m1, wz, torch.zeros_like(wz)))
        all3 = (True, True, True)
        g = grads_of(comp[:3], leaf, (wx, wv, wz), all3)
        want = grads_of(dense[:3], leaf_d, w_d, all3)
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
        assert torch.equal(g, want), (cap, float((g - want).abs().max()))
        assert bits(g, grads_of(comp[:3], leaf, (wx, wv, wz), all3))                             # the same bits from run to run
        for use in ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (True, False, True)):
            alone = grads_of(comp[:3], leaf, (wx, wv, wz), use)
            assert bool(torch.isfinite(alone).all()) and torch.equal(alone, grads_of(dense[:3], leaf_d, w_d, use)), (cap, use)


# ------------------------------------------------------------------------------------------------ 6. C ABI
CAN, PAD = 12345.5, 256


def banded(n, dev, dtype=torch.float32, can=CAN, fill=float("nan")):
    t = torch.full((n + PAD,), can, dtype=dtype, device=dev)
    t[:n] = fill
    return t


def test_abi_writes_every_element_and_nothing_else(amd, dev):
    ops, lib = amd.ops, amd._lib.lib()
    Nb, Nr, S = 3, 300, 5
    c = make_case(amd, Nb, Nr, S, seed=4)
    cam = R.cam2obj_of(c["poses"]).to(dev).contiguous()
    ins = [cam, c["wlh"].to(dev), c["rois"].to(dev), c["pixels"].to(dev)]
    jit = c["jitter"].to(dev)
    st = ops._stream(dev)
    dense = kernel(amd, dev, c)
    top = int(dense[3].sum(0).max())
    cap = ops.scene_capacity(top) + 32
    assert top > 32

    hit = banded(Nr * Nb, dev, torch.uint8, 77, 55)
    assert lib.snr_scene_pair_hits(*[ops._p(t) for t in ins], *c["Kvec"], Nr, Nb, 1, ops._p(hit), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(hit[:Nr * Nb], dense[3].reshape(-1)) and bool((hit[Nr * Nb:] == 77).all())
    keep = hit.clone()
    assert lib.snr_scene_pair_hits(*[ops._p(t) for t in ins], *c["Kvec"], 0, Nb, 1, ops._p(hit), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(hit, keep)

    for capacity in (cap, 32):       # roomy (padding on every object) and short (pairs dropped)
        want = RC.scene_samples_compact(dense, dense[3], capacity, S)
        scan = want["scan"].contiguous()
        n3, nz, nk, ns = Nb * capacity * S * 3, Nr * Nb * S, Nr * Nb, Nb * capacity
        xyz, viewdir, z = banded(n3, dev), banded(n3, dev), banded(nz, dev)
        kept, pos = banded(nk, dev, torch.uint8, 77, 55), banded(ns, dev, torch.int32, 4242, -7)

        def fwd(n_pixels):
            return lib.snr_scene_samples_compact_fwd(*[ops._p(t) for t in ins], *c["Kvec"], ops._p(jit), n_pixels, Nb, S, 1.0, 1, 1, ops._p(scan), capacity,
                                                     ops._p(xyz), ops._p(viewdir), ops._p(z), ops._p(kept), ops._p(pos), st)
        assert fwd(Nr) == 0
        torch.cuda.synchronize()
        for t, n, ref in ((xyz, n3, want["xyz"]), (viewdir, n3, want["viewdir"]), (z, nz, want["z_vals"])):
            assert not bool(torch.isnan(t[:n]).any()) and bits(t[:n], ref.reshape(-1)) and bool((t[n:] == CAN).all())
        assert torch.equal(kept[:nk].bool(), want["kept"].reshape(-1)) and bool((kept[nk:] == 77).all())
        assert torch.equal(pos[:ns], want["pair_of_slot"].reshape(-1)) and bool((pos[ns:] == 4242).all())
        # no pixel: padding only, the pixel-major outputs untouched
        for t in (xyz, viewdir):
            t[:n3] = float("nan")
        pos[:ns] = -7
        z_keep, kept_keep = z.clone(), kept.clone()
        assert fwd(0) == 0
        torch.cuda.synchronize()
        assert bool((xyz[:n3] == 0).all()) and bool((viewdir[:n3].view(-1, 3) == torch.tensor([0.0, 0.0, 1.0], device=dev)).all())
        assert bool((pos[:ns] == -1).all()) and torch.equal(z, z_keep) and torch.equal(kept, kept_keep)
        assert bool((xyz[n3:] == CAN).all()) and bool((viewdir[n3:] == CAN).all()) and bool((pos[ns:] == 4242).all())

        # backward: the 12 * Nb numbers and nothing else; each upstream gradient may be missing
        wx, wv, wz = upstream(c, capacity, want["pair_of_slot"], 8, dev)
        n_ws = int(lib.snr_scene_samples_bwd_ws_bytes(Nr, Nb))
        ws = torch.full((n_ws // 8 + PAD,), CAN, dtype=torch.float64, device=dev)
        out = banded(12 * Nb, dev)

        def bwd(n_pixels, grads):
            return lib.snr_scene_samples_compact_bwd(*[ops._p(t) for t in ins], *c["Kvec"], ops._p(jit), n_pixels, Nb, S, 1.0, 1, 1, ops._p(scan), capacity,
                                                     *[ops._p(t) for t in grads], ops._p(out), ops._p(ws), n_ws, st)
        assert bwd(Nr, (wx, wv, wz)) == 0
        torch.cuda.synchronize()
        leaf = cam.clone().requires_grad_()
        ref = grads_of(run_compact(amd, dev, c, capacity, scan, leaf)[:3], leaf, (wx, wv, wz), (True, True, True))
        assert bits(out[:12 * Nb], ref.reshape(-1)) and bool((out[12 * Nb:] == CAN).all()) and bool((ws[n_ws // 8:] == CAN).all())
        assert bwd(Nr, (None, None, None)) == 0
        torch.cuda.synchronize()
        assert bool((out[:12 * Nb] == 0).all())
        out.fill_(CAN)
        assert bwd(0, (wx, wv, wz)) == 0
        torch.cuda.synchronize()
        assert bool((out == CAN).all())

        # gather: either output may be missing
        kept8 = want["kept"].to(torch.uint8).contiguous()
        slots = want["pair_of_slot"].contiguous()
        sig, rgb = torch.randn(Nb * capacity * S, device=dev), torch.rand(Nb * capacity * S, 3, device=dev)
        g_s, g_r = banded(nz, dev), banded(nz * 3, dev)
        call = lambda s_in, r_in, n, s_out, r_out: lib.snr_scene_gather_compact_fwd(ops._p(s_in), ops._p(r_in), ops._p(scan), ops._p(kept8), n, Nb, S,
                                                                                    capacity, ops._p(s_out), ops._p(r_out), st)
        assert call(sig, rgb, Nr, g_s, g_r) == 0
        torch.cuda.synchronize()
        ref_s, ref_r = RC.gather_compact(sig, rgb, want["slot"], want["kept"], S)
        assert bits(g_s[:nz], ref_s.reshape(-1)) and bits(g_r[:nz * 3], ref_r.reshape(-1))
        assert bool((g_s[nz:] == CAN).all()) and bool((g_r[nz * 3:] == CAN).all())
        keep_s = g_s.clone()
        g_r.fill_(CAN)
        assert call(sig, None, Nr, g_s, None) == 0 and call(sig, rgb, 0, g_s, g_r) == 0
        torch.cuda.synchronize()
        assert torch.equal(g_s, keep_s) and bool((g_r == CAN).all())
        g_s.fill_(CAN)
        assert call(None, rgb, Nr, None, g_r) == 0
        torch.cuda.synchronize()
        assert bits(g_r[:nz * 3], ref_r.reshape(-1)) and bool((g_s == CAN).all())

        d_s, d_r = torch.randn(Nr, Nb * S, device=dev), torch.randn(Nr, Nb * S, 3, device=dev)
        nc = Nb * capacity * S
        o_s, o_r = banded(nc, dev), banded(nc * 3, dev)
        back = lambda s_in, r_in, s_out, r_out: lib.snr_scene_gather_compact_bwd(ops._p(s_in), ops._p(r_in), ops._p(slots), Nr, Nb, S, capacity,
                                                                                 ops._p(s_out), ops._p(r_out), st)
        assert back(d_s, d_r, o_s, o_r) == 0
        torch.cuda.synchronize()
        ref_s, ref_r = RC.gather_compact_bwd(d_s, d_r, want["pair_of_slot"], S)
        assert bits(o_s[:nc], ref_s) and bits(o_r[:nc * 3], ref_r.reshape(-1)) and bool((o_s[nc:] == CAN).all()) and bool((o_r[nc * 3:] == CAN).all())
        keep_s = o_s.clone()
        o_r.fill_(CAN)
        assert back(d_s, None, o_s, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(o_s, keep_s) and bool((o_r == CAN).all())
        o_s.fill_(CAN)
        assert back(None, d_r, None, o_r) == 0
        torch.cuda.synchronize()
        assert bits(o_r[:nc * 3], ref_r.reshape(-1)) and bool((o_s == CAN).all())


def test_lists_are_never_an_index(amd, dev):
    """A scan, kept flags and slot list full of junk: every launch stays inside its buffers (guard bands) and finishes."""
    ops, lib = amd.ops, amd._lib.lib()
    Nb, Nr, S, cap = 3, 300, 5, 32
    c = make_case(amd, Nb, Nr, S, seed=4)
    ins = [R.cam2obj_of(c["poses"]).to(dev).contiguous(), c["wlh"].to(dev), c["rois"].to(dev), c["pixels"].to(dev)]
    st = ops._stream(dev)
    gen = torch.Generator().manual_seed(0)
    junk = torch.randint(-2 ** 31, 2 ** 31 - 1, (Nr, Nb), generator=gen, dtype=torch.int64).to(torch.int32)
    junk[::3] = torch.randint(-40, 40, (Nr, Nb), generator=gen, dtype=torch.int64).to(torch.int32)[::3]
    junk[-1] = torch.tensor([2 ** 31 - 1, -5, 7], dtype=torch.int32)
    junk = junk.to(dev)
    n3, nz, nk, ns = Nb * cap * S * 3, Nr * Nb * S, Nr * Nb, Nb * cap
    xyz, viewdir, z = banded(n3, dev), banded(n3, dev), banded(nz, dev)
    kept, pos = banded(nk, dev, torch.uint8, 77, 55), banded(ns, dev, torch.int32, 4242, -7)
    assert lib.snr_scene_samples_compact_fwd(*[ops._p(t) for t in ins], *c["Kvec"], None, Nr, Nb, S, 1.0, 1, 1, ops._p(junk), cap, ops._p(xyz),
                                             ops._p(viewdir), ops._p(z), ops._p(kept), ops._p(pos), st) == 0
    torch.cuda.synchronize()
    assert bool((xyz[n3:] == CAN).all()) and bool((viewdir[n3:] == CAN).all()) and bool((z[nz:] == CAN).all())
    assert bool((kept[nk:] == 77).all()) and bool((pos[ns:] == 4242).all()) and not bool(torch.isnan(z[:nz]).any())
    out, n_ws = banded(12 * Nb, dev), int(lib.snr_scene_samples_bwd_ws_bytes(Nr, Nb))
    ws = torch.full((n_ws // 8 + PAD,), CAN, dtype=torch.float64, device=dev)
    w3, wz = torch.ones(n3, device=dev), torch.ones(nz, device=dev)
    assert lib.snr_scene_samples_compact_bwd(*[ops._p(t) for t in ins], *c["Kvec"], None, Nr, Nb, S, 1.0, 1, 1, ops._p(junk), cap, ops._p(w3), ops._p(w3),
                                             ops._p(wz), ops._p(out), ops._p(ws), n_ws, st) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[:12 * Nb]).all()) and bool((out[12 * Nb:] == CAN).all()) and bool((ws[n_ws // 8:] == CAN).all())
    flags = torch.randint(0, 256, (Nr, Nb), generator=gen).to(torch.uint8).to(dev)
    sig, rgb = torch.ones(Nb * cap * S, device=dev), torch.ones(Nb * cap * S, 3, device=dev)
    g_s, g_r = banded(nz, dev), banded(nz * 3, dev)
    assert lib.snr_scene_gather_compact_fwd(ops._p(sig), ops._p(rgb), ops._p(junk), ops._p(flags), Nr, Nb, S, cap, ops._p(g_s), ops._p(g_r), st) == 0
    torch.cuda.synchronize()
    assert bool(((g_s[:nz] == 0) | (g_s[:nz] == 1)).all()) and bool((g_r[:nz * 3] == 1).all()) and bool((g_s[nz:] == CAN).all()) and bool((g_r[nz * 3:] == CAN).all())
    slots = torch.randint(-2 ** 31, 2 ** 31 - 1, (Nb, cap), generator=gen, dtype=torch.int64).to(torch.int32)
    slots[:, ::2] = torch.randint(-3, Nr + 3, (Nb, cap), generator=gen, dtype=torch.int64).to(torch.int32)[:, ::2]
    slots = slots.to(dev)
    d_s, d_r = torch.ones(Nr, Nb * S, device=dev), torch.ones(Nr, Nb * S, 3, device=dev)
    nc = Nb * cap * S
    o_s, o_r = banded(nc, dev), banded(nc * 3, dev)
    assert lib.snr_scene_gather_compact_bwd(ops._p(d_s), ops._p(d_r), ops._p(slots), Nr, Nb, S, cap, ops._p(o_s), ops._p(o_r), st) == 0
    torch.cuda.synchronize()
    assert bool(((o_s[:nc] == 0) | (o_s[:nc] == 1)).all()) and bool((o_s[nc:] == CAN).all()) and bool((o_r[nc * 3:] == CAN).all())


# ------------------------------------------------------------------------------------------------ 7. render_scene(compact=True)
def compact_with_grads(amd, dev, s, pixels, jitter, w, capacity=None, info=None):
    g = s["g"]
    poses = g["obj_poses"].to(dev).requires_grad_()
    sc, tc = g["shapecodes"].to(dev).requires_grad_(), g["texturecodes"].to(dev).requires_grad_()
    out = amd.scene.render_scene(s["model"], dev, poses, g["obj_wlh"], sc, tc, g["K"], pixels, s["H"], s["W"], s["S"], jitter=jitter, fused=True,
                                 compact=True, capacity=capacity, info=info)
    grads = torch.autograd.grad(sum((o * wi.to(dev)).sum() for o, wi in zip(out, w)), (poses, sc, tc))
    return [t.detach().double().cpu() for t in (*out, *grads)]


def test_render_scene_compact_against_fused(amd, dev, scene):
    """Outputs and gradients to poses and both codes on the fixture's 300 pixels: compact against fused, in the band test_scene_rows_gpu.py
    builds for fused against default (4 x default route fp32 - float64 poses, floor one ulp)."""
    idx, Ws = scene["idx"], scene["W"]
    pixels = torch.stack([idx % Ws, idx // Ws], 1)
    jitter = scene["g"]["jitter"][:idx.numel() * 3].contiguous().to(dev)
    gen = torch.Generator().manual_seed(5)
    w = (torch.randn(idx.numel(), 3, generator=gen), torch.randn(idx.numel(), generator=gen), torch.randn(idx.numel(), generator=gen))
    d32 = render_with_grads(amd, dev, scene, pixels, jitter, w)
    d64 = render_with_grads(amd, dev, scene, pixels, jitter, w, dtype=torch.float64)
    fus = render_with_grads(amd, dev, scene, pixels, jitter, w, fused=True)
    info = {}
    com = compact_with_grads(amd, dev, scene, pixels, jitter, w, info=info)
    g = scene["g"]
    count = amd.ops.SceneSamples.apply(amd.scene.U.invert_pose(g["obj_poses"]).float().to(dev), g["obj_wlh"].to(dev),
                                       amd.scene.scene_rois(g["obj_poses"].float(), g["obj_wlh"], g["K"], scene["H"], Ws).to(dev),
                                       pixels.to(dev, torch.int32), amd.scene.K_vector(g["K"]), None, scene["S"], 1.0, True, True)[3].sum(0).cpu()
    assert info["count"].dtype == torch.int32 and info["count"].cpu().tolist() == count.tolist()
    assert info["capacity"] == amd.ops.scene_capacity(int(count.max())) and int(count.min()) >= 150
    print("render_scene compact: forward bit-equal to fused:", all(torch.equal(a, b) for a, b in zip(com[:3], fus[:3])), "capacity", info["capacity"],
          "counts", count.tolist())
    bad = []
    for name, a, b, f, k in zip(("rgb", "depth", "acc_trans", "d_poses", "d_shapecodes", "d_texturecodes"), d32, d64, fus, com):
        band = max(4 * float((a - b).abs().max()), ulp_of(a))
        err = float((k - f).abs().max())
        print(f"render_scene {name}: compact - fused {err:.3e}, band {band:.3e} (fp32 - float64 poses {band / 4:.3e}), largest {float(a.abs().max()):.3e}")
        assert bool(torch.isfinite(k).all()), name
        if not err <= band:
            bad.append((name, err, band))
    assert not bad, bad
    # a given capacity makes no read and, when it holds every hit, changes nothing; one too small renders the surplus as misses
    info2 = {}
    roomy = compact_with_grads(amd, dev, scene, pixels, jitter, w, capacity=info["capacity"] + 32, info=info2)
    assert info2["capacity"] == info["capacity"] + 32 and all(torch.equal(a, b) for a, b in zip(roomy[:3], com[:3]))
    short = compact_with_grads(amd, dev, scene, pixels, jitter, w, capacity=32, info=info2)
    assert all(bool(torch.isfinite(t).all()) for t in short) and info2["count"].cpu().tolist() == count.tolist()
    assert not torch.equal(short[0], com[0])
    with torch.no_grad():       # without grad mode: the same values
        g = scene["g"]
        plain = amd.scene.render_scene(scene["model"], dev, g["obj_poses"], g["obj_wlh"], g["shapecodes"], g["texturecodes"], g["K"], pixels,
                                       scene["H"], scene["W"], scene["S"], jitter=jitter, fused=True, compact=True)
    assert all(torch.equal(a.double().cpu(), b) for a, b in zip(plain, com[:3]))


# ------------------------------------------------------------------------------------------------ 8. optimize_scene(compact=True)
def fit(amd, dev, s, **kw):
    info = {}
    out = amd.driver.optimize_scene(s["model"], dev, s["frame"], s["hp"], s["g"]["shapecodes"], s["g"]["texturecodes"], pose_noise=NOISE, seed=SEED,
                                    jitter=s["jitter"], pixels=s["pixels"], info=info, **kw)
    return out, info


def test_optimize_scene_compact_against_dense(amd, dev, setup):
    """compact=True against compact=False in the setup of tests/test_scene_fit_gpu.py, held to its band: 4 x the distance between the twin loop
    with fp32 and with float64 pose leaves, floor one fp32 ulp."""
    s = setup
    (m0, l0, sc0, tc0, p0), i0 = fit(amd, dev, s)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        (m1, l1, sc1, tc1, p1), i1 = fit(amd, dev, s, compact=True)
    assert not [w for w in caught if "capacity" in str(w.message)]
    Nr, Nb = s["pixels"].shape[0], s["g"]["obj_poses"].shape[0]
    assert "capacity" not in i0 and "dropped_pairs" not in i0
    assert i1["capacity"] % 32 == 0 and 32 <= i1["capacity"] <= amd.ops.scene_capacity(Nr) and int(i1["dropped_pairs"]) == 0
    assert i1["dropped_pairs"].is_cuda and i1["hit_share"].shape == (T,)
    assert float((i1["hit_share"] - i0["hit_share"])[0].abs()) <= 1e-6 and 0 < float(i1["hit_share"].min()) <= float(i1["hit_share"].max()) < 1
    assert m1.shape == (T, Nb, 2) and l1.shape == (T, 4) and all(p.requires_grad for p in s["model"].parameters())
    t32, ok32 = twin(amd, dev, s, torch.float32)
    t64, ok64 = twin(amd, dev, s, torch.float64)
    assert ok32 and ok64
    bad = []
    for name, k, f, a, b in zip(("loss per iteration", "poses", "shape codes", "texture codes"), (l1[:, 0], p1, sc1, tc1), (l0[:, 0], p0, sc0, tc0), t32, t64):
        k, f = k.double().cpu(), f.double().cpu()
        top = float(a.abs().max())
        band = max(4 * float((a - b).abs().max()), float(np.finfo(np.float32).eps) * 2.0 ** np.floor(np.log2(top)))
        err = float((k - f).abs().max())
        print(f"optimize_scene {name}: compact - dense {err:.3e}, band {band:.3e} (twin fp32 - float64 leaves {band / 4:.3e}), largest {top:.3e}")
        assert bool(torch.isfinite(k).all()), name
        if not err <= band:
            bad.append((name, err, band))
    assert not bad, bad
    # the measured default: the fullest object at the start poses times the margin
    (_, _, _, _, _), i2 = fit(amd, dev, s, compact=True, capacity_margin=100.0)
    assert i2["capacity"] == amd.ops.scene_capacity(Nr)
    # a capacity that cannot hold the hits: a warning, a count, finite results
    with pytest.warns(RuntimeWarning, match="capacity"):
        (m3, l3, sc3, tc3, p3), i3 = fit(amd, dev, s, compact=True, capacity=32)
    assert i3["capacity"] == 32 and int(i3["dropped_pairs"]) > 0
    assert all(bool(torch.isfinite(t).all()) for t in (m3, l3, sc3, tc3, p3))
    assert float((i3["hit_share"] - i0["hit_share"][0]).abs()[0]) <= 1e-6                       # the geometric share, dropped pairs included
    with pytest.raises(amd.SnrError, match="compact"):
        fit(amd, dev, s, capacity=32)
