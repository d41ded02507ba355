"""GPU tests of the scene sample kernels (snr_scene_samples_fwd / bwd, snr_scene_gather_fwd / bwd) behind ``ops.SceneSamples`` /
``ops.SceneGather``, of ``scene.render_pairs`` (the one fused chain) and of ``scene.render_scene(fused=True)``.

The oracle of record is the float64 run of tests/scene_rows_restatement.py.  No band below is fixed in advance and no code under test enters
one: per output it is 4 x the worst absolute error of the EXISTING fp32 torch route (``scene.scene_ray_rows`` + the sample lines of
``scene.render_scene_batch``, run on the host) against float64 on the compared pairs, with a floor of one fp32 ulp of the output's largest
magnitude.  A pair is left out of the value comparison only if it is a float64 hit whose slab gap far - near is below 1e-3 (a grazing ray) or
if the fp32 route's and the float64 hit flags differ; at most 1 % of a case's pairs may be left out, and on all others the kernel's flag must
equal both."""
import pytest
import torch

import scene_rows_restatement as R
from oracle_bands import amd, dev, make_model  # noqa: F401  (amd, dev: fixtures)

pytestmark = pytest.mark.gpu

H, W = 60, 160
ULP = float(torch.finfo(torch.float32).eps)


def ulp_of(t):
    """One fp32 ulp at the largest magnitude of ``t``."""
    top = float(t.abs().max())
    return ULP * 2.0 ** torch.floor(torch.log2(torch.tensor(max(top, 1e-30)))).item()


def make_case(amd, Nb, Nr, S, seed, rend_aabb=True, shapenet=True, scale=1.0, jitter=True):
    """Nb synthetic objects in one 60 x 160 camera, turned a little out of their axis-parallel yaw planes; Nr pixels drawn from the union of
    the rois (nine in ten) and from the whole image."""
    gen = torch.Generator().manual_seed(seed)
    f = amd.synthetic.synthetic_frame(list(range(seed, seed + Nb)), H, W, focal=0.45 * W if Nb <= 3 else 0.3 * W)
    dR = amd.driver.axis_angle_to_matrix(torch.randn(Nb, 3, generator=gen) * 0.2)
    poses = torch.cat([dR @ f["obj_poses"][:, :, :3], f["obj_poses"][:, :, 3:]], dim=2).contiguous()
    rois = amd.scene.scene_rois(poses, f["obj_wlh"], f["K"], H, W)
    cover = torch.zeros(H, W, dtype=torch.bool)
    for x0, y0, x1, y1 in rois.tolist():
        cover[y0:max(y1, y0), x0:max(x1, x0)] = True
    ys, xs = torch.nonzero(cover, as_tuple=True)
    pick = torch.randint(0, ys.numel(), (Nr,), generator=gen)
    pixels = torch.stack([xs[pick], ys[pick]], 1)
    anywhere = torch.rand(Nr, generator=gen) < 0.1
    pixels[anywhere] = torch.stack([torch.randint(0, W, (Nr,), generator=gen), torch.randint(0, H, (Nr,), generator=gen)], 1)[anywhere]
    K = f["K"]
    return dict(poses=poses, wlh=f["obj_wlh"], K=K, Kvec=(float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])), rois=rois,
                pixels=pixels.to(torch.int32), jitter=torch.rand(Nr * Nb, S, generator=gen) if jitter else None, S=S, scale=scale,
                rend_aabb=rend_aabb, shapenet=shapenet, Nb=Nb, Nr=Nr)


def kernel(amd, dev, c, cam2obj=None, pixels=None, jitter="case"):
    cam2obj = R.cam2obj_of(c["poses"]).to(dev) if cam2obj is None else cam2obj
    jit = c["jitter"] if isinstance(jitter, str) else jitter
    return amd.ops.SceneSamples.apply(cam2obj, c["wlh"].to(dev), c["rois"].to(dev), (c["pixels"] if pixels is None else pixels).to(dev), c["Kvec"],
                                      None if jit is None else jit.to(dev), c["S"], c["scale"], c["rend_aabb"], c["shapenet"])


def oracle(c, dtype, leaf=False):
    cam2obj = R.cam2obj_of(c["poses"].to(dtype))
    if leaf:
        cam2obj = cam2obj.detach().requires_grad_()
    return cam2obj, R.scene_samples(cam2obj, c["wlh"], c["rois"], c["pixels"], c["Kvec"], c["jitter"], c["S"], c["scale"], c["rend_aabb"], c["shapenet"])


def route32(amd, c, poses=None):
    return R.existing_route(amd.scene, c["poses"] if poses is None else poses, c["wlh"], c["K"], c["pixels"].long(), H, W, c["jitter"], c["S"],
                            c["scale"], c["rend_aabb"], c["shapenet"])


def check_forward(amd, dev, c, name):
    xyz, viewdir, z, hit, valid = kernel(amd, dev, c)
    got = dict(xyz=xyz.cpu(), viewdir=viewdir.cpu(), z_vals=z.cpu())
    hit, valid = hit.cpu().bool(), valid.cpu().bool()
    _, o64 = oracle(c, torch.float64)
    r32 = route32(amd, c)
    S, Nb, Nr = c["S"], c["Nb"], c["Nr"]
    assert got["xyz"].shape == (Nb * Nr, S, 3) and got["viewdir"].shape == (Nb * Nr, S, 3) and got["z_vals"].shape == (Nr, Nb * S)
    excluded = (o64["hit"] & (o64["gap"] < 1e-3)) | (r32["hit"] != o64["hit"])
    share = float(excluded.float().mean())
    print(f"{name}: {int(o64['hit'].sum())} of {hit.numel()} pairs hit, {int(excluded.sum())} excluded")
    assert share <= 0.01, (name, share)
    assert torch.equal(hit[~excluded], o64["hit"][~excluded]) and torch.equal(hit[~excluded], r32["hit"][~excluded])
    assert torch.equal(valid[~excluded.any(1)], o64["valid"][~excluded.any(1)])
    # pairs that are not hit hold the stated constants exactly
    m3, m1 = R.pair_mask(hit, S)
    assert bool((got["z_vals"][~m1] == -1).all()) and bool((got["xyz"][~m3] == 0).all())
    assert torch.equal(got["viewdir"][~m3].view(-1, 3), torch.tensor([0.0, 0.0, 1.0]).expand(int((~m3).sum()) // 3, 3))
    c3, c1 = R.pair_mask(o64["hit"] & hit & ~excluded, S)
    worst = {}
    for k, m in (("xyz", c3), ("viewdir", c3), ("z_vals", c1)):
        assert bool(torch.isfinite(got[k]).all()), k
        if not bool(m.any()):
            continue
        ref = o64[k][m]
        band = max(4 * float((r32[k].double()[m] - ref).abs().max()), ulp_of(ref))
        err = float((got[k].double()[m] - ref).abs().max())
        print(f"{name} {k}: kernel {err:.3e}, band {band:.3e} (fp32 route {band / 4:.3e}, ulp {ulp_of(ref):.3e})")
        worst[k] = (err, band)
    bad = {k: v for k, v in worst.items() if not v[0] <= v[1]}
    assert not bad, (name, bad)
    return hit


SHAPES = [(1, 1, 16), (1, 63, 1), (1, 300, 64), (3, 64, 2), (3, 65, 16), (3, 300, 16), (3, 1025, 65), (8, 1, 64), (8, 63, 16), (8, 64, 65),
          (8, 300, 64), (8, 1025, 2), (3, 257, 1)]
#         Nr crosses the 256-pixel slice at 257, 300 and 1025 (five slices, the last one pixel); S = 65 is no power of two


@pytest.mark.parametrize("Nb,Nr,S", SHAPES)
def test_forward_in_band(amd, dev, Nb, Nr, S):
    check_forward(amd, dev, make_case(amd, Nb, Nr, S, seed=Nb + Nr + S), f"({Nb},{Nr},{S})")


@pytest.mark.parametrize("variant", ["sphere", "object_frame", "scaled", "no_jitter"])
def test_forward_variants(amd, dev, variant):
    kw = dict(sphere=dict(rend_aabb=False), object_frame=dict(shapenet=False), scaled=dict(scale=0.6), no_jitter=dict(jitter=False))[variant]
    c = make_case(amd, 3, 300, 16, seed=5, **kw)
    hit = check_forward(amd, dev, c, variant)
    if variant == "sphere":       # every covered pair hits
        assert torch.equal(hit, oracle(c, torch.float64)[1]["covered"])


def hand_case(amd):
    """Four objects in the 60 x 160 camera: 0 and 1 ordinary, 2 behind the camera (its roi handed in as if it covered the image), 3 with the
    identity rotation on the optical axis; a dead roi is swapped in for object 1 by the caller."""
    c = make_case(amd, 4, 16, 16, seed=9)
    poses = c["poses"].clone()
    poses[2, :, 3] = torch.tensor([0.0, 0.0, -12.0])
    poses[3] = torch.cat([torch.eye(3), torch.tensor([[0.1], [-0.05], [9.0]])], dim=1)
    c["poses"] = poses
    rois = amd.scene.scene_rois(poses, c["wlh"], c["K"], H, W)
    rois[2] = torch.tensor([0, 0, W - 1, H - 1], dtype=torch.int32)
    c["rois"] = rois
    return c


def test_hand_placed_pairs(amd, dev):
    c = hand_case(amd)
    x0, y0, x1, y1 = c["rois"][0].tolist()
    cx, cy = int(c["Kvec"][2]), int(c["Kvec"][3])
    assert c["Kvec"][2] == cx and c["Kvec"][3] == cy
    px = [(x0, y0), (x1 - 1, y1 - 1), (x1, y0), (x0, y1), (x0 - 1, y0), (x0, y0 - 1), (-1, 5), (W, 5), (5, -1), (5, H), (W + 1000, H + 1000),
          (cx, cy), ((x0 + x1) // 2, (y0 + y1) // 2), (-2 ** 31, 2 ** 31 - 1), (cx + 1, cy), tuple((c["rois"][1, :2] + c["rois"][1, 2:]).div(2, rounding_mode="floor").tolist())]
    c["pixels"] = torch.tensor(px, dtype=torch.int64).to(torch.int32)
    hit = check_forward(amd, dev, c, "hand")
    _, o64 = oracle(c, torch.float64)
    cov = o64["covered"]
    assert cov[0, 0] and cov[1, 0] and not cov[2, 0] and not cov[3, 0] and not cov[4, 0] and not cov[5, 0]      # x0, y0 inside; x1, y1 outside
    assert not bool(cov[6:11].any()) and not bool(cov[13].any()) and not bool(hit[6:11].any()) and not bool(hit[13].any())   # outside the image
    assert bool(cov[:, 2].any()) and not bool(hit[:, 2].any())                   # behind the camera: covered by the roi handed in, never hit
    assert bool(hit[11, 3])                                                       # the principal point through the identity object
    u = R.cam2obj_of(c["poses"])[3, :, :3] @ torch.tensor([0.0, 0.0, 1.0])
    assert u.tolist() == [0.0, 0.0, 1.0]                                          # two direction components are exactly 0
    # a dead roi: nothing of that object is hit, the others are untouched
    assert bool(hit[:, 1].any())
    d = dict(c)
    d["rois"] = c["rois"].clone()
    d["rois"][1] = torch.tensor([40, 10, 40, 30], dtype=torch.int32)
    live, dead = [t.cpu() for t in kernel(amd, dev, c)], [t.cpu() for t in kernel(amd, dev, d)]
    assert not bool(dead[3][:, 1].any()) and torch.equal(dead[3][:, [0, 2, 3]], live[3][:, [0, 2, 3]]) and torch.equal(dead[4], dead[3].any(1).to(torch.uint8))
    Nr, S = c["Nr"], c["S"]
    for b in (0, 2, 3):
        for i in (0, 1):
            assert torch.equal(dead[i][b * Nr:(b + 1) * Nr], live[i][b * Nr:(b + 1) * Nr])
        assert torch.equal(dead[2].view(Nr, -1, S)[:, b], live[2].view(Nr, -1, S)[:, b])
    assert bool((dead[2].view(Nr, -1, S)[:, 1] == -1).all()) and bool((dead[0][Nr:2 * Nr] == 0).all())


# ------------------------------------------------------------------------------------------------ backward
def weights(c, seed):
    gen = torch.Generator().manual_seed(seed)
    n = c["Nb"] * c["Nr"] * c["S"]
    return torch.randn(n // c["S"], c["S"], 3, generator=gen), torch.randn(n // c["S"], c["S"], 3, generator=gen), torch.randn(c["Nr"], c["Nb"] * c["S"], generator=gen)


def loss_of(out, w, use=(True, True, True)):
    return sum((o * wi.to(o.device, o.dtype)).sum() for o, wi, u in zip(out, w, use) if u)


def kernel_grads(amd, dev, c, w, use=(True, True, True), pixels=None, jitter="case", w_perm=None):
    """(d_cam2obj through ops.SceneSamples, d_obj_poses through the two torch ops in front of it)"""
    poses = c["poses"].detach().clone().to(dev).requires_grad_()
    cam2obj = R.cam2obj_of(poses)
    cam2obj.retain_grad()
    out = kernel(amd, dev, c, cam2obj, pixels, jitter)[:3]
    loss_of(out, w if w_perm is None else w_perm, use).backward()
    return cam2obj.grad.cpu(), poses.grad.cpu()


def backward_bands(amd, c, w):
    """float64 autograd of the restatement (d_cam2obj, d_poses), and the relative band: 4 x the distance of the existing fp32 route's autograd
    from float64, floor one ulp.  The existing route has no cam2obj leaf (it derives it from the object poses), so its distance is taken
    on d(obj_poses), relative to the largest float64 entry, and held against both gradients."""
    p64 = c["poses"].double().requires_grad_()
    cam64 = R.cam2obj_of(p64)
    cam64.retain_grad()
    o = R.scene_samples(cam64, c["wlh"], c["rois"], c["pixels"], c["Kvec"], c["jitter"], c["S"], c["scale"], c["rend_aabb"], c["shapenet"])
    loss_of((o["xyz"], o["viewdir"], o["z_vals"]), w).backward()
    p32 = c["poses"].clone().requires_grad_()
    r = route32(amd, c, p32)
    # (the fp32 route's samples on pairs that are not hit are thrown away downstream: they carry no upstream gradient)
    m3, m1 = R.pair_mask(r["hit"], c["S"])
    loss_of((torch.where(m3, r["xyz"], torch.zeros_like(r["xyz"])), torch.where(m3, r["viewdir"], torch.zeros_like(r["viewdir"])),
             torch.where(m1, r["z_vals"], torch.zeros_like(r["z_vals"]))), w).backward()
    assert torch.equal(r["hit"], o["hit"]), "the backward cases are chosen without grazing pairs"
    top = float(p64.grad.abs().max())
    rel = max(4 * float((p32.grad.double() - p64.grad).abs().max()) / top, ULP)
    return cam64.grad, p64.grad, rel


BWD_CASES = [(1, 63, 16, "box"), (3, 300, 16, "box"), (8, 65, 64, "box"), (3, 1025, 2, "box"), (8, 300, 65, "box"), (3, 64, 1, "box"),
             (3, 300, 16, "sphere"), (8, 65, 64, "sphere"), (3, 300, 16, "object_frame_scaled"), (8, 65, 64, "object_frame_scaled")]


@pytest.mark.parametrize("Nb,Nr,S,variant", BWD_CASES)
def test_backward_in_band(amd, dev, Nb, Nr, S, variant):
    kw = dict(box={}, sphere=dict(rend_aabb=False), object_frame_scaled=dict(shapenet=False, scale=0.6))[variant]
    c = make_case(amd, Nb, Nr, S, seed=3 * Nb + Nr + S, **kw)
    w = weights(c, Nr)
    g64, p64, rel = backward_bands(amd, c, w)
    g, p = kernel_grads(amd, dev, c, w)
    assert bool(torch.isfinite(g).all())
    e_g = float((g.double() - g64).abs().max()) / float(g64.abs().max())
    e_p = float((p.double() - p64).abs().max()) / float(p64.abs().max())
    print(f"({Nb},{Nr},{S}) {variant}: d_cam2obj {e_g:.3e}, d_poses {e_p:.3e}, band {rel:.3e} (fp32 route {rel / 4:.3e})")
    assert e_g <= rel and e_p <= rel, (e_g, e_p, rel)
    # the same bits from run to run
    g2, _ = kernel_grads(amd, dev, c, w)
    assert torch.equal(g, g2)
    # each gradient alone, the others null == the others passed as zeros
    for i in range(3):
        use = tuple(j == i for j in range(3))
        alone, _ = kernel_grads(amd, dev, c, w, use)
        zeros = tuple(wi if u else torch.zeros_like(wi) for wi, u in zip(w, use))
        with_zeros, _ = kernel_grads(amd, dev, c, zeros)
        assert torch.equal(alone, with_zeros), i
        assert float(alone.abs().max()) > 0
    # a permuted pixel list: the same sums in another order
    perm = torch.randperm(Nr, generator=torch.Generator().manual_seed(1))
    jit = None if c["jitter"] is None else c["jitter"].view(Nr, Nb, S)[perm].reshape(Nr * Nb, S)
    w_perm = (w[0].view(Nb, Nr, S, 3)[:, perm].reshape(Nb * Nr, S, 3), w[1].view(Nb, Nr, S, 3)[:, perm].reshape(Nb * Nr, S, 3), w[2][perm])
    gp, _ = kernel_grads(amd, dev, c, w, pixels=c["pixels"][perm], jitter=jit, w_perm=w_perm)
    assert float((gp.double() - g64).abs().max()) / float(g64.abs().max()) <= rel


def test_backward_zero_direction_components(amd, dev):
    """The identity object through the principal point: u = (0,0,1); the two parallel axes add nothing and nothing is NaN."""
    c = hand_case(amd)
    cx, cy = int(c["Kvec"][2]), int(c["Kvec"][3])
    c["pixels"] = torch.tensor([(cx, cy)] * 2 + [(cx + 1, cy), (cx, cy - 1)], dtype=torch.int32)
    c["Nr"], c["jitter"] = 4, c["jitter"][:4 * c["Nb"]]
    w = weights(c, 2)
    g, p = kernel_grads(amd, dev, c, w)
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(p).all()) and float(g[3].abs().max()) > 0
    assert bool(oracle(c, torch.float64)[1]["hit"][0, 3])
    g64, _, rel = backward_bands(amd, c, w)
    assert bool(torch.isfinite(g64).all())
    err = float((g.double() - g64).abs().max()) / float(g64.abs().max())
    print(f"zero components: d_cam2obj {err:.3e}, band {rel:.3e}")
    assert err <= rel
    assert float(g[2].abs().max()) == 0        # the object behind the camera is never hit: exact zeros


# ------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("Nb,Nr,S", [(1, 1, 1), (3, 65, 16), (8, 300, 65), (3, 1025, 2)])
def test_gather_is_the_torch_ops(amd, dev, Nb, Nr, S):
    gen = torch.Generator().manual_seed(Nr)
    sig, rgb = torch.randn(Nb * Nr * S, generator=gen).to(dev), torch.rand(Nb * Nr * S, 3, generator=gen).to(dev)
    hit = (torch.rand(Nr, Nb, generator=gen) < 0.5).to(torch.uint8).to(dev)
    ws, wr = torch.randn(Nr, Nb * S, generator=gen).to(dev), torch.randn(Nr, Nb * S, 3, generator=gen).to(dev)
    res = []
    for fn in (lambda a, b: amd.ops.SceneGather.apply(a, b, hit, S), lambda a, b: R.gather(a, b, hit, S)):
        a, b = sig.clone().requires_grad_(), rgb.clone().requires_grad_()
        out = fn(a, b)
        res.append((out, torch.autograd.grad((out[0] * ws).sum() + (out[1] * wr).sum(), (a, b)), torch.autograd.grad((fn(a, b)[0] * ws).sum(), (a,))))
    for mine, theirs in zip(res[0], res[1]):
        for x, y in zip(mine, theirs):
            assert x.shape == y.shape and torch.equal(x, y)
    # the decoder's (N,S,1) / (N,S,3) shapes pass as they are
    a = amd.ops.SceneGather.apply(sig.view(Nb * Nr, S, 1), rgb.view(Nb * Nr, S, 3), hit, S)
    assert torch.equal(a[0], res[0][0][0]) and torch.equal(a[1], res[0][0][1])


# ------------------------------------------------------------------------------------------------ C ABI
CAN, PAD = 12345.5, 256


def test_abi_writes_every_element_and_nothing_else(amd, dev):
    ops, lib = amd.ops, amd._lib.lib()
    c = make_case(amd, 3, 300, 5, seed=4)
    Nb, Nr, S = 3, 300, 5
    cam = R.cam2obj_of(c["poses"]).to(dev).contiguous()
    ins = [cam, c["wlh"].to(dev), c["rois"].to(dev), c["pixels"].to(dev)]
    jit = c["jitter"].to(dev)
    want = kernel(amd, dev, c)
    sizes = dict(xyz=Nb * Nr * S * 3, viewdir=Nb * Nr * S * 3, z=Nr * Nb * S)
    f = {k: torch.full((n + PAD,), CAN, device=dev) for k, n in sizes.items()}
    for k, n in sizes.items():
        f[k][:n] = float("nan")
    b = {k: torch.full((n + PAD,), 77, dtype=torch.uint8, device=dev) for k, n in (("hit", Nr * Nb), ("valid", Nr))}

    def fwd(n_pixels, valid):
        return lib.snr_scene_samples_fwd(*[ops._p(t) for t in ins], *c["Kvec"], ops._p(jit), n_pixels, Nb, S, 1.0, 1, 1, ops._p(f["xyz"]),
                                         ops._p(f["viewdir"]), ops._p(f["z"]), ops._p(b["hit"]), ops._p(valid), ops._stream(dev))
    assert fwd(Nr, b["valid"]) == 0
    torch.cuda.synchronize()
    for k, ref in zip(("xyz", "viewdir", "z"), want[:3]):
        assert not bool(torch.isnan(f[k][:sizes[k]]).any()) and torch.equal(f[k][:sizes[k]], ref.reshape(-1)) and bool((f[k][sizes[k]:] == CAN).all())
    assert torch.equal(b["hit"][:Nr * Nb], want[3].reshape(-1)) and bool((b["hit"][Nr * Nb:] == 77).all())
    assert torch.equal(b["valid"][:Nr], want[4]) and bool((b["valid"][Nr:] == 77).all())
    # valid is optional; no pixel is no launch
    b["valid"].fill_(77)
    assert fwd(Nr, None) == 0
    for t in list(f.values()) + [b["hit"]]:
        t.fill_(55)
    assert fwd(0, b["valid"]) == 0
    torch.cuda.synchronize()
    assert all(bool((t == 55).all()) for t in list(f.values()) + [b["hit"]]) and bool((b["valid"] == 77).all())

    # backward: the 12 * Nb numbers and nothing else; each upstream gradient may be missing
    w = [t.to(dev).contiguous() for t in weights(c, 8)]
    n_ws = int(lib.snr_scene_samples_bwd_ws_bytes(Nr, Nb))
    ws = torch.empty(n_ws // 8 + PAD, dtype=torch.float64, device=dev).fill_(CAN)
    out = torch.full((12 * Nb + PAD,), CAN, device=dev)
    out[:12 * Nb] = float("nan")

    def bwd(n_pixels, grads):
        return lib.snr_scene_samples_bwd(*[ops._p(t) for t in ins], *c["Kvec"], ops._p(jit), n_pixels, Nb, S, 1.0, 1, 1, *[ops._p(t) for t in grads],
                                         ops._p(out), ops._p(ws), n_ws, ops._stream(dev))
    assert bwd(Nr, w) == 0
    torch.cuda.synchronize()
    leaf = cam.clone().requires_grad_()
    loss_of(kernel(amd, dev, c, leaf)[:3], w).backward()
    assert torch.equal(out[:12 * Nb], leaf.grad.reshape(-1))
    assert bool((out[12 * Nb:] == CAN).all()) and bool((ws[n_ws // 8:] == CAN).all())
    assert bwd(Nr, [None, None, None]) == 0
    torch.cuda.synchronize()
    assert bool((out[:12 * Nb] == 0).all())
    out.fill_(CAN)
    assert bwd(0, w) == 0
    torch.cuda.synchronize()
    assert bool((out == CAN).all())

    # gather: either output may be missing
    sig, rgb = torch.randn(Nb * Nr * S, device=dev), torch.rand(Nb * Nr * S, 3, device=dev)
    for name in ("snr_scene_gather_fwd", "snr_scene_gather_bwd"):
        g_s, g_r = torch.full((Nr * Nb * S + PAD,), CAN, device=dev), torch.full((Nr * Nb * S * 3 + PAD,), CAN, device=dev)
        g_s[:Nr * Nb * S] = float("nan"); g_r[:Nr * Nb * S * 3] = float("nan")
        assert getattr(lib, name)(ops._p(sig), ops._p(rgb), ops._p(want[3]), Nr, Nb, S, ops._p(g_s), ops._p(g_r), ops._stream(dev)) == 0
        torch.cuda.synchronize()
        assert not bool(torch.isnan(g_s).any()) and not bool(torch.isnan(g_r).any())
        assert bool((g_s[Nr * Nb * S:] == CAN).all()) and bool((g_r[Nr * Nb * S * 3:] == CAN).all())
        if name.endswith("fwd"):
            ref_s, ref_r = R.gather(sig, rgb, want[3], S)
            assert torch.equal(g_s[:Nr * Nb * S], ref_s.reshape(-1)) and torch.equal(g_r[:Nr * Nb * S * 3], ref_r.reshape(-1))
        keep = g_s.clone()
        g_r.fill_(CAN)
        assert getattr(lib, name)(ops._p(sig), ops._p(None), ops._p(want[3]), Nr, Nb, S, ops._p(g_s), ops._p(None), ops._stream(dev)) == 0
        assert getattr(lib, name)(ops._p(sig), ops._p(rgb), ops._p(want[3]), 0, Nb, S, ops._p(g_s), ops._p(g_r), ops._stream(dev)) == 0
        torch.cuda.synchronize()
        assert torch.equal(g_s, keep) and bool((g_r == CAN).all())


# ------------------------------------------------------------------------------------------------ render_pairs
def test_render_pairs_is_the_four_ops_by_hand(amd, dev, oracle_params):
    """``scene.render_pairs`` against SceneSamples -> decoder -> SceneGather -> composite written out here, bit for bit: 257 pixels (one more
    than a 256-pair slice), two objects of which one has a dead roi, 4 samples; under ``no_grad`` (``ops.scene_composite``) and with
    ``cam2obj`` and both codes requiring a gradient (``ops.SceneComposite``), there with the three gradients of one backward."""
    ops = amd.ops
    Nb, Nr, S = 2, 257, 4
    c = make_case(amd, Nb, Nr, S, seed=21)
    rois = c["rois"].clone()
    assert bool(((rois[:, 2] > rois[:, 0]) & (rois[:, 3] > rois[:, 1])).all())
    rois[1] = torch.tensor([40, 10, 40, 30], dtype=torch.int32)                  # dead: x1 == x0
    model = make_model(amd, dev, oracle_params, "fp32")
    gen = torch.Generator().manual_seed(22)
    sc0, tc0 = torch.randn(Nb, 256, generator=gen) * 0.3, torch.randn(Nb, 256, generator=gen) * 0.3
    w = (torch.randn(Nr, 3, generator=gen).to(dev), torch.randn(Nr, generator=gen).to(dev), torch.randn(Nr, generator=gen).to(dev))
    wlh, rois, pixels, jitter = c["wlh"].to(dev), rois.to(dev), c["pixels"].to(dev), c["jitter"].to(dev)

    def leaves(grad):
        return [t.to(dev).requires_grad_(grad) for t in (R.cam2obj_of(c["poses"]), sc0, tc0)]

    def by_hand(cam2obj, sc, tc, composite):
        xyz, viewdir, z, hit, _ = ops.SceneSamples.apply(cam2obj, wlh, rois, pixels, c["Kvec"], jitter, S, c["scale"], c["rend_aabb"], c["shapenet"])
        sig, rgb = model(xyz, viewdir, sc, tc)
        sig, rgb = ops.SceneGather.apply(sig, rgb, hit, S)
        return (*composite(sig, rgb, z), hit)

    def pairs(cam2obj, sc, tc):
        return amd.scene.render_pairs(lambda x, d: model(x, d, sc, tc), cam2obj, wlh, rois, pixels, c["Kvec"], jitter, S, c["scale"], c["rend_aabb"],
                                      c["shapenet"])
    with torch.no_grad():
        want = by_hand(*leaves(False), lambda sig, rgb, z: ops.scene_composite(sig, rgb, z, white_bkgd=True, run_length=S))
        got = pairs(*leaves(False))
    assert len(got) == 4 and got[3].shape == (Nr, Nb) and got[3].dtype == torch.uint8
    assert bool(got[3][:, 0].any()) and not bool(got[3][:, 1].any())             # the live object is hit, the dead roi never
    for name, a, b in zip(("rgb", "depth", "acc", "hit"), got, want):
        assert not a.requires_grad and a.shape == b.shape and torch.equal(a, b), name
    plain = got
    res = []
    for fn in (lambda *l: by_hand(*l, lambda sig, rgb, z: ops.SceneComposite.apply(sig, rgb, z, True, S)), pairs):
        lv = leaves(True)
        out = fn(*lv)
        assert out[0].requires_grad and not out[3].requires_grad
        sum((o * wi).sum() for o, wi in zip(out[:3], w)).backward()
        res.append([t.detach() for t in out] + [t.grad for t in lv])
    for name, a, b in zip(("rgb", "depth", "acc", "hit", "d_cam2obj", "d_shapecodes", "d_texturecodes"), res[1], res[0]):
        assert a.shape == b.shape and torch.equal(a, b), name
    assert all(torch.equal(a, b) for a, b in zip(res[1][:4], plain))             # either composite branch: the same values
    g_cam, g_sc, g_tc = res[1][4:]
    assert float(g_cam[0].abs().max()) > 0 and float(g_sc[0].abs().max()) > 0 and float(g_tc[0].abs().max()) > 0
    assert float(g_cam[1].abs().max()) == 0 and float(g_sc[1].abs().max()) == 0 and float(g_tc[1].abs().max()) == 0


# ------------------------------------------------------------------------------------------------ render_scene(fused=True)
@pytest.fixture(scope="module")
def scene(amd, dev, golden, oracle_params):
    """The scene fixture's 300 pixels as tests/test_scene_grad_gpu.py picks them: the 150 that hit all three objects and 150 of the others."""
    g = golden("scene")
    Hs, Ws = int(g["H"]), int(g["W"])
    table, valid, _ = amd.scene.scene_rays(g["obj_poses"], g["obj_wlh"], g["K"], Hs, Ws)
    table = table.view(Hs * Ws, -1, 8)
    hit = (table[..., 7] - table[..., 6]) > 0
    all3 = torch.nonzero(hit.all(1)).flatten()
    assert all3.numel() == 150
    others = torch.nonzero(valid & ~hit.all(1)).flatten()
    others = others[torch.linspace(0, others.numel() - 1, 150).long()]
    idx = torch.cat([all3, others])
    return dict(g=g, H=Hs, W=Ws, table=table, hit=hit, idx=idx, model=make_model(amd, dev, oracle_params, "fp32"), S=16)


def render_with_grads(amd, dev, s, pixels, jitter, w, dtype=torch.float32, fused=False):
    g = s["g"]
    poses = g["obj_poses"].to(dev, dtype).requires_grad_()
    sc, tc = g["shapecodes"].to(dev).requires_grad_(), g["texturecodes"].to(dev).requires_grad_()
    out = amd.scene.render_scene(s["model"], dev, poses, g["obj_wlh"], sc, tc, g["K"], pixels, s["H"], s["W"], s["S"], jitter=jitter, fused=fused)
    grads = torch.autograd.grad(sum((o * wi.to(dev)).sum() for o, wi in zip(out, w)), (poses, sc, tc))
    return [t.detach().double().cpu() for t in (*out, *grads)]


def test_render_scene_fused_against_default(amd, dev, scene):
    """Outputs and gradients to poses and both codes: the fused route against the default one, held to 4 x the distance between the default
    route with fp32 poses and with float64 poses (``scene_ray_rows`` works in the poses' dtype), same jitter; floor one fp32 ulp of the
    tensor's largest magnitude."""
    idx, Ws = scene["idx"], scene["W"]
    pixels = torch.stack([idx % Ws, idx // Ws], 1)
    jitter = scene["g"]["jitter"][:idx.numel() * 3].contiguous().to(dev)
    gen = torch.Generator().manual_seed(5)
    w = (torch.randn(idx.numel(), 3, generator=gen), torch.randn(idx.numel(), generator=gen), torch.randn(idx.numel(), generator=gen))
    d32 = render_with_grads(amd, dev, scene, pixels, jitter, w)
    d64 = render_with_grads(amd, dev, scene, pixels, jitter, w, dtype=torch.float64)
    fus = render_with_grads(amd, dev, scene, pixels, jitter, w, fused=True)
    bad = []
    for name, a, b, f in zip(("rgb", "depth", "acc_trans", "d_poses", "d_shapecodes", "d_texturecodes"), d32, d64, fus):
        band = max(4 * float((a - b).abs().max()), ulp_of(a))
        err = float((f - a).abs().max())
        print(f"render_scene {name}: fused - default {err:.3e}, band {band:.3e} (fp32 - float64 poses {band / 4:.3e}), largest {float(a.abs().max()):.3e}")
        assert bool(torch.isfinite(f).all()), name
        if not err <= band:
            bad.append((name, err, band))
    assert not bad, bad


def test_render_scene_fused_untouched_object(amd, dev, scene):
    """An object whose roi holds none of the listed pixels gets exact zero gradients; the others get some."""
    table, hit, Ws = scene["table"], scene["hit"], scene["W"]
    in_roi = ~(table == -1).all(-1)
    pick = None
    for b in range(in_roi.shape[1]):
        cand = torch.nonzero(~in_roi[:, b] & hit.any(1)).flatten()
        if cand.numel() >= 12:
            pick = (b, cand[torch.linspace(0, cand.numel() - 1, 12).long()])
            break
    assert pick is not None
    away, idx = pick
    pixels = torch.stack([idx % Ws, idx // Ws], 1)
    gen = torch.Generator().manual_seed(6)
    w = (torch.randn(12, 3, generator=gen), torch.randn(12, generator=gen), torch.randn(12, generator=gen))
    jitter = scene["g"]["jitter"][:36].contiguous().to(dev)
    out = render_with_grads(amd, dev, scene, pixels, jitter, w, fused=True)
    for t in out[3:]:
        assert bool(torch.isfinite(t).all()) and float(t[away].abs().max()) == 0
    covering = [b for b in range(in_roi.shape[1]) if b != away and bool(hit[idx, b].any())]
    assert covering and all(float(out[3][b].abs().max()) > 0 and float(out[4][b].abs().max()) > 0 for b in covering)
    with torch.no_grad():       # without grad mode: the same values
        g = scene["g"]
        plain = amd.scene.render_scene(scene["model"], dev, g["obj_poses"], g["obj_wlh"], g["shapecodes"], g["texturecodes"], g["K"], pixels,
                                       scene["H"], scene["W"], scene["S"], jitter=jitter, fused=True)
    assert all(torch.equal(a.double().cpu(), b) for a, b in zip(plain, out[:3]))
