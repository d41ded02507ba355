"""GPU tests of the differentiable scene render: snr_scene_composite_bwd behind ``ops.SceneComposite`` against the dense restatement
(tests/scene_grad_restatement.py) in float64, its bit-level seams (one list == ``ops.Composite``, permutations, two runs, canaries through
the C ABI), its limits, and the wiring through ``scene.render_scene_batch`` / ``scene.render_scene`` down to codes, ray rows and poses."""
import pytest
import torch

import scene_grad_restatement as R
from oracle_bands import amd, dev, check_all, make_model  # noqa: F401  (amd, dev: fixtures)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 64, 37), (3, 64, 101), (4, 64, 57), (2, 128, 40), (4, 32, 77), (8, 32, 33), (7, 33, 50), (2, 5, 300), (8, 64, 20),
          (1, 5, 1), (3, 85, 9), (4, 64, 5), (1, 257, 4), (2, 32, 33000)]
#          n = 5       n = 255     n = 256     n = 257      more pixels than the launch has waves (8192 workgroups x 4): the grid-stride loop runs


def weights(P, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(P, 3, generator=gen), torch.randn(P, generator=gen), torch.randn(P, generator=gen)


def kernel_grads(amd, dev, sig, rgb, z, w, white=True, run=0):
    """(d_sigma, d_rgb, d_z) of sum(w_rgb rgb) + sum(w_depth depth) + sum(w_acc acc) through ops.SceneComposite; a None weight leaves
    that output unused (its incoming gradient is None)."""
    a, b, c = [t.to(dev).requires_grad_() for t in (sig, rgb, z)]
    out = amd.ops.SceneComposite.apply(a, b, c, white, run)
    loss = sum((o * wi.to(dev)).sum() for o, wi in zip(out, w) if wi is not None)
    return torch.autograd.grad(loss, (a, b, c))


def against_restatement(amd, dev, sig, rgb, z, w, white, got, name):
    chunk = 1024 if z.shape[1] <= 64 else 256
    o64 = R.grads(sig, rgb, z, *w, white_bkgd=white, dtype=torch.float64, chunk=chunk)
    o32 = R.grads(sig, rgb, z, *w, white_bkgd=white, dtype=torch.float32, chunk=chunk)
    check_all([(f"{name} d_{k}", g, a, b) for k, g, a, b in zip(("sigma", "rgb", "z"), got, o32, o64)], "fp32")


@pytest.mark.parametrize("quarters", [False, True])
@pytest.mark.parametrize("Nb,S,P", SHAPES)
def test_kernel_against_restatement(amd, dev, Nb, S, P, quarters):
    sig, rgb, z = R.shape_case(Nb, S, P, quarters)
    w = weights(P, P + Nb)
    g0 = kernel_grads(amd, dev, sig, rgb, z, w, True, 0)
    gS = kernel_grads(amd, dev, sig, rgb, z, w, True, S)
    for a, b in zip(g0, gS):
        assert torch.equal(a, b)                      # the hint only changes how the ranks are found
    if P > 8192 * 4:                                  # the grid-stride launch: the values under grad mode are the plain forward's
        assert all(torch.equal(a, b) for a, b in zip(amd.ops.SceneComposite.apply(*[t.to(dev).requires_grad_() for t in (sig, rgb, z)], True, S),
                                                     amd.ops.scene_composite(sig.to(dev), rgb.to(dev), z.to(dev), True, S)))
    against_restatement(amd, dev, sig, rgb, z, w, True, g0, f"({Nb},{S},{P}){' quarters' if quarters else ''}")


@pytest.mark.parametrize("Nb,S,P", [(3, 64, 101), (7, 33, 50), (1, 257, 4)])
def test_kernel_variants(amd, dev, Nb, S, P):
    """Lists reversed under the hint S (a wrong hint: the answer of hint 0), black background, depth and acc outputs unused."""
    sig, rgb, z = R.shape_case(Nb, S, P)
    w = weights(P, 7 * P)
    n = Nb * S
    zr = z.view(P, Nb, S).flip(-1).reshape(P, n).contiguous()
    g0 = kernel_grads(amd, dev, sig, rgb, zr, w, True, 0)
    gS = kernel_grads(amd, dev, sig, rgb, zr, w, True, S)
    for a, b in zip(g0, gS):
        assert torch.equal(a, b)
    against_restatement(amd, dev, sig, rgb, zr, w, True, gS, "reversed lists")
    for white in (False, True):
        for ww in ((w[0], None, None), (w[0], w[1], None), (w[0], None, w[2])):
            got = kernel_grads(amd, dev, sig, rgb, z, ww, white, S)
            against_restatement(amd, dev, sig, rgb, z, ww, white, got, f"white={white} unused={[k for k, x in zip(('rgb', 'depth', 'acc'), ww) if x is None]}")


# ------------------------------------------------------------------------------------------------ bit-level seams
@pytest.mark.parametrize("white", [True, False])
@pytest.mark.parametrize("S", [2, 5, 64, 65, 256])
def test_one_list_is_the_plain_composite(amd, dev, S, white):
    """One ascending tie-free list: the merge is the identity and both kernels run composite_ray_bwd on the same sequence."""
    gen = torch.Generator().manual_seed(S)
    P = 23
    z = (2 + torch.sort(torch.rand(P, S, generator=gen) * 4, dim=-1)[0])
    assert bool((z[:, 1:] > z[:, :-1]).all())
    sig, rgb = torch.rand(P, S, generator=gen) * 2 - 0.3, torch.rand(P, S, 3, generator=gen)
    w = weights(P, S)
    a, b, c = [t.to(dev).requires_grad_() for t in (sig, rgb, z)]
    out = amd.ops.Composite.apply(a, b, c, amd.ops.Z_PER_RAY, white, 0)
    want = torch.autograd.grad(sum((o * wi.to(dev)).sum() for o, wi in zip(out, w)), (a, b, c))
    for run in (0, S):
        got = kernel_grads(amd, dev, sig, rgb, z, w, white, run)
        for x, y in zip(got, want):
            assert torch.equal(x, y)


@pytest.mark.parametrize("n", [48, 200, 300, 512])
def test_permutation_and_determinism(amd, dev, n):
    gen = torch.Generator().manual_seed(n)
    P = 19
    # distinct depths by construction (n uniform draws in fp32 do collide): a shuffled grid of spacing 6 / n, jittered by less than half of it
    z = 2 + (torch.argsort(torch.rand(P, n, generator=gen), dim=1) + 0.4 * torch.rand(P, n, generator=gen)) * (6.0 / n)
    assert bool(R.tie_free(z).all())
    sig, rgb = torch.rand(P, n, generator=gen) * 2 - 0.3, torch.rand(P, n, 3, generator=gen)
    w = weights(P, n)
    base = kernel_grads(amd, dev, sig, rgb, z, w)
    again = kernel_grads(amd, dev, sig, rgb, z, w)
    for x, y in zip(base, again):
        assert torch.equal(x, y)
    perm = torch.argsort(torch.rand(P, n, generator=gen), dim=1)               # another order per pixel
    take = lambda t: torch.gather(t, 1, perm if t.dim() == 2 else perm[:, :, None].expand(-1, -1, 3))   # noqa: E731
    got = kernel_grads(amd, dev, take(sig), take(rgb), take(z), w)
    for x, y in zip(got, base):
        assert torch.equal(x.cpu(), take(y.cpu()))


@pytest.mark.parametrize("P,n,run", [(3, 10, 5), (5, 257, 0)])
def test_abi_writes_every_element_and_nothing_else(amd, dev, P, n, run):
    """Caller-owned buffers with canaries behind the three outputs: every element written, no canary touched."""
    ops = amd.ops
    sig, rgb, z = R.shape_case(1, n, P) if run == 0 else R.shape_case(n // run, run, P, quarters=True)
    w = weights(P, 3)
    CAN, PAD = 12345.5, 256
    bufs = {k: torch.full((P * n * c + PAD,), CAN, device=dev) for k, c in (("sig", 1), ("rgb", 3), ("z", 1))}
    for k, c in (("sig", 1), ("rgb", 3), ("z", 1)):
        bufs[k][:P * n * c] = float("nan")
    ins = [t.to(dev).contiguous() for t in (sig, rgb, z)]
    ws = [t.to(dev).contiguous() for t in w]
    rc = amd._lib.lib().snr_scene_composite_bwd(ops._p(ins[0]), ops._p(ins[1]), ops._p(ins[2]), P, n, run, ops.WHITE_BKGD, ops._p(ws[0]), ops._p(ws[1]),
                                                ops._p(ws[2]), ops._p(bufs["sig"]), ops._p(bufs["rgb"]), ops._p(bufs["z"]), ops._stream(dev))
    assert rc == 0
    torch.cuda.synchronize()
    want = kernel_grads(amd, dev, sig, rgb, z, w, True, run)
    for (k, c), ref in zip((("sig", 1), ("rgb", 3), ("z", 1)), want):
        body, tail = bufs[k][:P * n * c], bufs[k][P * n * c:]
        assert not bool(torch.isnan(body).any())
        assert torch.equal(body, ref.reshape(-1))
        assert bool((tail == CAN).all())
    # d_z is optional: without it the other two are the same and nothing else is written
    bufs["sig"].fill_(CAN); bufs["rgb"].fill_(CAN)
    rc = amd._lib.lib().snr_scene_composite_bwd(ops._p(ins[0]), ops._p(ins[1]), ops._p(ins[2]), P, n, run, ops.WHITE_BKGD, ops._p(ws[0]), ops._p(ws[1]),
                                                ops._p(ws[2]), ops._p(bufs["sig"]), ops._p(bufs["rgb"]), ops._p(None), ops._stream(dev))
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(bufs["sig"][:P * n], want[0].reshape(-1)) and torch.equal(bufs["rgb"][:P * n * 3], want[1].reshape(-1))
    assert bool((bufs["sig"][P * n:] == CAN).all()) and bool((bufs["rgb"][P * n * 3:] == CAN).all())


# ------------------------------------------------------------------------------------------------ limits
def test_limits(amd, dev):
    ops = amd.ops
    sig, rgb, z = [t.to(dev) for t in R.shape_case(1, 513, 3)]
    with pytest.raises(amd.SnrError, match="512"):
        ops.SceneComposite.apply(sig.clone().requires_grad_(), rgb, z, True, 0)
    with pytest.raises(amd.SnrError, match="512"):
        ops.scene_composite_bwd(sig, rgb, z, True, 0, torch.ones(3, 3, device=dev))
    plain = ops.scene_composite(sig, rgb, z, True, 0)
    for a, b in zip(ops.SceneComposite.apply(sig, rgb, z, True, 0), plain):
        assert torch.equal(a, b)
    with pytest.raises(amd.SnrError):
        ops.SceneComposite.apply(sig[:, :8].cpu().requires_grad_(), rgb[:, :8].cpu(), z[:, :8].cpu(), True, 0)
    with pytest.raises(amd.SnrError):
        ops.scene_composite_bwd(sig[:, :8].cpu(), rgb[:, :8].cpu(), z[:, :8].cpu(), True, 0, torch.ones(3, 3))
    with pytest.raises(amd.SnrError):
        ops.scene_composite_bwd(sig[:, :8].contiguous(), rgb[:, :8].contiguous(), z[:, :8].contiguous(), True, 3, torch.ones(3, 3, device=dev))
    e = ops.scene_composite_bwd(torch.zeros(0, 8, device=dev), torch.zeros(0, 8, 3, device=dev), torch.zeros(0, 8, device=dev), True, 0,
                                torch.zeros(0, 3, device=dev))
    assert e[0].shape == (0, 8) and e[1].shape == (0, 8, 3) and e[2].shape == (0, 8)


# ------------------------------------------------------------------------------------------------ wiring
@pytest.fixture(scope="module")
def scene(amd, dev, golden, oracle_params):
    g = golden("scene")
    H, W = int(g["H"]), int(g["W"])
    table, valid, diags = amd.scene.scene_rays(g["obj_poses"], g["obj_wlh"], g["K"], H, W)
    table = table.view(H * W, -1, 8)
    hit = (table[..., 7] - table[..., 6]) > 0
    all3 = torch.nonzero(hit.all(1)).flatten()
    assert all3.numel() == 150
    others = torch.nonzero(valid & ~hit.all(1)).flatten()
    others = others[torch.linspace(0, others.numel() - 1, 150).long()]
    idx = torch.cat([all3, others])
    model = make_model(amd, dev, oracle_params, "fp32")
    return dict(g=g, H=H, W=W, table=table, hit=hit, idx=idx, diags=diags, model=model, S=16, jitter=g["jitter"][:idx.numel() * 3].contiguous())


def test_render_scene_batch_wiring(amd, dev, scene, monkeypatch):
    g, model, S, diags = scene["g"], scene["model"], scene["S"], scene["diags"]
    batch = scene["table"][scene["idx"]]
    with torch.no_grad():
        ref = amd.scene.render_scene_batch(model, dev, batch, diags, g["shapecodes"], g["texturecodes"], S, scene["jitter"])
        ref_dev_jitter = amd.scene.render_scene_batch(model, dev, batch, diags, g["shapecodes"], g["texturecodes"], S, scene["jitter"].to(dev))
    for a, b in zip(ref, ref_dev_jitter):
        assert torch.equal(a, b)                      # a jitter that lives on the device: the same values

    seen = []
    real = amd.ops.SceneComposite

    class Tap:
        @staticmethod
        def apply(sig, rgb, z, white, run):
            seen.append((sig, rgb, z, white, run))
            return real.apply(sig, rgb, z, white, run)
    monkeypatch.setattr(amd.ops, "SceneComposite", Tap)
    sc, tc = g["shapecodes"].to(dev).requires_grad_(), g["texturecodes"].to(dev).requires_grad_()
    rows = batch.to(dev).requires_grad_()
    out = amd.scene.render_scene_batch(model, dev, rows, diags, sc, tc, S, scene["jitter"])
    monkeypatch.undo()
    assert len(seen) == 1 and seen[0][3] is True and seen[0][4] == S
    for a, b in zip(out, ref):
        assert torch.equal(a, b)

    # the kernel on decoder-made values (real dynamic range, saturated last intervals), as leaves
    P = rows.shape[0]
    w = weights(P, 11)
    sig, rgb, z = seen[0][:3]
    leaves = [t.detach().cpu() for t in (sig, rgb, z)]
    k = kernel_grads(amd, dev, *leaves, w, True, S)
    against_restatement(amd, dev, *leaves, w, True, k, "decoder-made")

    # the whole call == the decoder's and the samplers' backward seeded with the kernel's gradients
    loss = sum((o * wi.to(dev)).sum() for o, wi in zip(out, w))
    whole = torch.autograd.grad(loss, (sc, tc, rows), retain_graph=True)
    seeded = torch.autograd.grad((sig, rgb, z), (sc, tc, rows), grad_outputs=k, retain_graph=True)
    seeded2 = torch.autograd.grad((sig, rgb, z), (sc, tc, rows), grad_outputs=k, retain_graph=True)
    for name, a, b, b2 in zip(("shapecodes", "texturecodes", "rows"), whole, seeded, seeded2):
        assert bool(torch.isfinite(a).all()), name
        spread = float((b - b2).abs().max())
        if spread == 0:
            assert torch.equal(a, b), (name, float((a - b).abs().max()))
        else:
            # the unchanged decoder backward is itself not bit-stable from run to run here: hold the comparison to 4x its own spread
            print(f"{name}: decoder backward run-to-run spread {spread:.3e}")
            assert float((a - b).abs().max()) <= 4 * spread, (name, float((a - b).abs().max()), spread)
    assert float(whole[0].abs().max()) > 0 and float(whole[1].abs().max()) > 0 and float(whole[2].abs().max()) > 0
    # rows of objects that miss the pixel carry nothing
    miss = (batch[..., 6] == -1) & (batch[..., 7] == -1)
    assert bool(miss.any()) and float(whole[2][miss.to(dev)].abs().max()) == 0


def test_render_scene(amd, dev, scene):
    g, model, S, H, W = scene["g"], scene["model"], scene["S"], scene["H"], scene["W"]
    S_ = amd.scene
    table, hit = scene["table"], scene["hit"]
    in_roi = ~(table == -1).all(-1)                                            # (H*W, Nb)
    # an object whose roi holds none of the chosen pixels, which another object covers
    pick = None
    for b in range(in_roi.shape[1]):
        cand = torch.nonzero(~in_roi[:, b] & hit.any(1)).flatten()
        if cand.numel() >= 12:
            pick = (b, cand[torch.linspace(0, cand.numel() - 1, 12).long()])
            break
    assert pick is not None
    away, idx = pick
    pixels = torch.stack([idx % W, idx // W], 1)
    covering = [b for b in range(in_roi.shape[1]) if b != away and bool(hit[idx, b].any())]
    assert covering
    jitter = g["jitter"][:idx.numel() * 3].contiguous().to(dev)
    poses = g["obj_poses"].to(dev).requires_grad_()
    sc, tc = g["shapecodes"].to(dev).requires_grad_(), g["texturecodes"].to(dev).requires_grad_()
    out = S_.render_scene(model, dev, poses, g["obj_wlh"], sc, tc, g["K"], pixels, H, W, S, jitter=jitter)
    rows, valid = S_.scene_ray_rows(poses, g["obj_wlh"], g["K"], pixels, H, W)
    assert rows.device.type == "cuda" and bool(valid.all())
    want = S_.render_scene_batch(model, dev, rows, scene["diags"], sc, tc, S, jitter)
    for a, b in zip(out, want):
        assert torch.equal(a, b)
    # ... and what the reference-style table renders there, up to the fp32 noise of the rows
    with torch.no_grad():
        tab = S_.render_scene_batch(model, dev, table[idx], scene["diags"], g["shapecodes"], g["texturecodes"], S, jitter)
    assert float((out[0].detach() - tab[0]).abs().max()) < 1e-2                          # (the same picture: two grey levels of 255)
    w = weights(idx.numel(), 5)
    d_pose, d_sc, d_tc = torch.autograd.grad(sum((o * wi.to(dev)).sum() for o, wi in zip(out, w)), (poses, sc, tc))
    for t in (d_pose, d_sc, d_tc):
        assert bool(torch.isfinite(t).all())
    assert float(d_pose[away].abs().max()) == 0 and float(d_sc[away].abs().max()) == 0 and float(d_tc[away].abs().max()) == 0
    for b in covering:
        assert float(d_pose[b].abs().max()) > 0 and float(d_sc[b].abs().max()) > 0
    with pytest.raises(amd.SnrError):
        S_.render_scene(model, dev, poses, g["obj_wlh"], sc[:2], tc, g["K"], pixels, H, W, S)
    with pytest.raises(amd.SnrError):
        S_.render_scene(model, dev, poses[:2], g["obj_wlh"], sc, tc, g["K"], pixels, H, W, S)
    with pytest.raises(amd.SnrError):
        S_.render_scene(model, dev, poses, g["obj_wlh"][:1], sc, tc, g["K"], pixels, H, W, S)
