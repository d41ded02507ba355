"""Timing of the differentiable scene render on one GPU: device events, medians of ``--reps`` calls, calls that are compared taken in turn.

  * the backward launch (``ops.scene_composite_bwd``, d_z included) beside the forward launch (``ops.scene_composite``) at P = 65 536
    pixels for (Nb, S) in (2, 64), (4, 64), (8, 64), (8, 32), on the test generator's depths (ascending lists, 30 % empty objects), with
    the hint ``run_length`` = S and without.  Bytes counted: 20 per sample in for the forward, 20 in and 20 out for the backward, 20 per
    pixel for the pixel rows on either side;
  * one forward + backward of ``scene.render_scene`` on the three objects of the ``scene`` fixture (every covered pixel, the fixture's
    sample count), the forward alone beside it;
  * a short loss trace: ``--steps`` steps of 2 cm down the gradient of the object translations, started 0.2 m off, against the render at
    the fixture's poses.

Prints one JSON line.

usage: python tools/scene_grad_time.py [--reps N] [--pixels P] [--steps K] [--commit SHA]"""
import torch

import geometry_common as C
from conftest import load_golden
from ray_surface_time import in_turn
from supnerf_amd import ops, scene

SHAPES = ((2, 64), (4, 64), (8, 64), (8, 32))


def pixels_case(P, Nb, S, dev, seed=0):
    gen = torch.Generator().manual_seed(seed)
    z = torch.rand(P, Nb, 1, generator=gen) * 20 + 2 + torch.sort(torch.rand(P, Nb, S, generator=gen), dim=-1)[0] * 4
    sig = torch.rand(P, Nb, S, generator=gen) * 2 - 0.3
    rgb = torch.rand(P, Nb, S, 3, generator=gen)
    empty = torch.rand(P, Nb, generator=gen) < 0.3
    z[empty] = -1; sig[empty] = 0; rgb[empty] = 1
    return sig.view(P, Nb * S).to(dev), rgb.view(P, Nb * S, 3).to(dev), z.view(P, Nb * S).to(dev)


def launch_rows(P, reps, dev):
    rows = []
    for Nb, S in SHAPES:
        sig, rgb, z = pixels_case(P, Nb, S, dev)
        n = Nb * S
        g = torch.Generator().manual_seed(1)
        d_rgb, d_depth, d_acc = [torch.randn(*s, generator=g).to(dev) for s in ((P, 3), (P,), (P,))]
        fns = [lambda: ops.scene_composite(sig, rgb, z, True, S), lambda: ops.scene_composite_bwd(sig, rgb, z, True, S, d_rgb, d_depth, d_acc, True),
               lambda: ops.scene_composite(sig, rgb, z, True, 0), lambda: ops.scene_composite_bwd(sig, rgb, z, True, 0, d_rgb, d_depth, d_acc, True)]
        with torch.no_grad():
            f_s, b_s, f_0, b_0 = in_turn(fns, reps)
        fwd_bytes, bwd_bytes = P * n * 20 + P * 20, P * n * 40 + P * 20
        rows.append({"Nb": Nb, "S": S, "n": n, "P": P, "fwd_ms": f_s, "bwd_ms": b_s, "bwd_over_fwd": round(b_s / f_s, 3),
                     "fwd_GBps": round(fwd_bytes / f_s / 1e6, 1), "bwd_GBps": round(bwd_bytes / b_s / 1e6, 1),
                     "no_hint": {"fwd_ms": f_0, "bwd_ms": b_0, "bwd_over_fwd": round(b_0 / f_0, 3)}})
        del sig, rgb, z
    return rows


def render_rows(model, reps, steps, dev):
    g = load_golden("scene")
    H, W, S = int(g["H"]), int(g["W"]), int(g["n_samples"])
    valid = scene.scene_rays(g["obj_poses"], g["obj_wlh"], g["K"], H, W)[1]
    idx = torch.nonzero(valid).flatten()
    pixels = torch.stack([idx % W, idx // W], 1)
    Nb = g["obj_poses"].shape[0]
    jitter = torch.rand(idx.numel() * Nb, S, generator=torch.Generator().manual_seed(2)).to(dev)
    sc, tc = g["shapecodes"].to(dev).requires_grad_(), g["texturecodes"].to(dev).requires_grad_()
    poses = g["obj_poses"].to(dev).requires_grad_()
    render = lambda p: scene.render_scene(model, dev, p, g["obj_wlh"], sc, tc, g["K"], pixels, H, W, S, jitter=jitter)      # noqa: E731
    with torch.no_grad():
        target = render(poses)[0]

    def fwd_only():
        with torch.no_grad():
            render(poses)

    def fwd_bwd():
        loss = ((render(poses)[0] - 0.5) ** 2).mean()
        torch.autograd.grad(loss, (poses, sc, tc))
    t_f, t_fb = in_turn([fwd_only, fwd_bwd], reps)
    # a loss trace: translations 0.2 m off along x, plain steps of 2 cm down the gradient of the translations.  (On the fog decoder of this
    # tool the loss is mostly silhouette pixels that an object gains or loses, which carry no gradient: the trace shows the plumbing, it
    # is no optimiser.)
    base = g["obj_poses"].to(dev)
    moved = lambda sh: torch.cat([base[:, :, :3], base[:, :, 3:4] + sh[:, :, None]], 2)      # noqa: E731
    loss_at = lambda sh: ((render(moved(sh))[0] - target) ** 2).mean()                      # noqa: E731
    shift = torch.zeros(Nb, 3, device=dev)
    shift[:, 0] = 0.2
    shift.requires_grad_()
    trace = []
    for _ in range(steps):
        loss = loss_at(shift)
        grad, = torch.autograd.grad(loss, shift)
        trace.append(round(float(loss.detach()), 6))
        with torch.no_grad():
            shift -= 0.02 * grad / grad.norm().clamp_min(1e-20)
    return {"pixels": int(idx.numel()), "objects": int(Nb), "S": S, "forward_ms": t_f, "forward_backward_ms": t_fb, "loss_trace": trace}


def main():
    a = C.arguments(C.BLOCKS, ("--pixels", dict(type=int, default=65536)), ("--steps", dict(type=int, default=10)))
    dev = torch.device("cuda:0")
    sb, tb = a.blocks
    model = C.fog_decoder(sb, tb, dev)
    C.report("scene_grad_time", a, (sb, tb), reps=a.reps, launches=launch_rows(a.pixels, a.reps, dev), render_scene=render_rows(model, a.reps, a.steps, dev))


if __name__ == "__main__":
    main()
