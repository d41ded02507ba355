"""Which ``ops`` entry points one iteration of ``driver._fit_views`` calls on each of its paths: the benchmarked batched loop makes none of
the multi-view calls, and the multi-view loop makes exactly its three.  The counters are host-side wrappers around the entry points; they
launch nothing themselves.  The expected numbers are read off the loop body (and were counted the same way on the two loop bodies this
one replaced)."""
import collections

import pytest
import torch

from oracle import supnerf_oracle as O
from oracle_bands import amd, dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(amd, dev):
    m = amd.CodeNeRF(3, 1)
    m.load_state_dict(O.init_decoder_params())
    m.precision = "fp32"                               # requested, so no probe renders anything
    return m.to(dev)


def count_calls(monkeypatch, ops):
    """Wrap the loop's entry points of ``ops`` with counters -> the Counter they fill.  ``FusedRender.forward`` and ``render_probe`` reach
    ``snr_render_fwd`` through the same module-level ``ops.render_fwd`` the depth render calls, so the wrapped function sees both: calls made
    while ``FusedRender.apply`` is running are counted as "render_fwd in FusedRender", the others as "render_fwd"."""
    n = collections.Counter()
    in_fused = []

    def wrap(owner, attr, key, static=False):
        real = getattr(owner, attr)

        def counting(*a, **k):
            n["render_fwd in FusedRender" if key == "render_fwd" and in_fused else key] += 1
            if key == "FusedRender":
                in_fused.append(1)
            try:
                return real(*a, **k)
            finally:
                if key == "FusedRender":
                    in_fused.pop()
        monkeypatch.setattr(owner, attr, staticmethod(counting) if static else counting)
    for name in ("instance_rows_fwd", "view_pixels", "render_fwd", "metric_row"):
        wrap(ops, name, name)
    for name in ("InstanceRows", "FusedRender", "LossTail", "PoseRays", "CamRays"):
        wrap(getattr(ops, name), "apply", name, static=True)            # (``apply`` is looked up on the class)
    wrap(ops.DeviceAdamW, "step", "DeviceAdamW.step")
    return n


def start_codes(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 256, generator=g) * 0.3, torch.randn(n, 256, generator=g) * 0.3


def batched_run(amd, D, dev, model, with_table):
    """B = 2 on the 8 x 8 grid, S = 16, T = 3, reg_iters = 1: iterations 0 and 1 only render, iteration 2 steps."""
    hp = D.load_hpams()
    hp["n_samples"], hp["render_im_sz"], hp["optimize"]["num_opts"] = 16, 8, 3
    objs = D.make_objects([3, 8], 8)
    table = None
    if with_table:                                     # (2, 2, 3, 4): the true object poses, the second entry shifted by a few centimetres
        gt = torch.stack([amd.utils.invert_pose(ob["cam_pose"]) for ob in objs])
        moved = gt.clone()
        moved[:, :, 3] += torch.tensor([0.05, -0.03, 0.08])
        table = torch.stack([gt, moved], dim=1)
    sc0, tc0 = start_codes(2, 1)
    jit = torch.rand(3, 2, 2, 16, generator=torch.Generator().manual_seed(2))
    info = {}
    m, *_ = D.optimize_objects_batched(model, dev, objs, hp, sc0, tc0, [11, 12], reg_iters=1, jitter=jit, info=info, pose_per_iter=table)
    assert m.shape == (2, 3, 4) and bool(torch.isfinite(m).all()) and list(info) == ["lidar_count"]


def multiview_run(D, dev, model, opt_pose):
    """I = 2 with V = (2, 1), 16 random native pixels per view and iteration, S = 16, T = 2."""
    hp = D.load_hpams()
    hp["n_samples"], hp["optimize"]["num_opts"] = 16, 2
    inst = [D.make_instances([4], 2)[0], D.make_instances([9], 1)[0]]
    sc0, tc0 = start_codes(2, 3)
    m, *_ = D.optimize_instances(model, dev, inst, hp, sc0, tc0, [21, 22, 23], opt_pose=opt_pose, sampling="random", n_rays=16)
    assert m.shape == (3, 2, 4) and bool(torch.isfinite(m).all())


@pytest.mark.parametrize("with_table", [False, True])
def test_batched_loop_makes_no_multiview_calls(amd, dev, model, monkeypatch, with_table):
    n = count_calls(monkeypatch, amd.ops)
    batched_run(amd, amd.driver, dev, model, with_table)
    print(dict(n))
    assert n["instance_rows_fwd"] == 0 and n["view_pixels"] == 0 and n["InstanceRows"] == 0
    assert n["FusedRender"] == 3 and n["LossTail"] == 3 and n["metric_row"] == 3
    assert n["render_fwd"] == 3 and n["render_fwd in FusedRender"] == 3       # the depth renders; one launch per FusedRender, no probe
    assert n["DeviceAdamW.step"] == 1
    # two ray launches per iteration (render, depth render): from the table in iterations 0 and 1, from the optimised pose otherwise
    assert (n["PoseRays"], n["CamRays"]) == ((2, 4) if with_table else (6, 0))


@pytest.mark.parametrize("opt_pose", [True, False])
def test_multiview_loop_call_counts(amd, dev, model, monkeypatch, opt_pose):
    T = 2
    n = count_calls(monkeypatch, amd.ops)
    multiview_run(amd.driver, dev, model, opt_pose)
    print(dict(n))
    assert n["view_pixels"] == T and n["InstanceRows"] == T
    assert n["instance_rows_fwd"] == 2 * T                                     # one inside InstanceRows, one for the latent biases
    assert n["FusedRender"] == T and n["LossTail"] == T and n["metric_row"] == T and n["DeviceAdamW.step"] == T
    assert n["render_fwd"] == T and n["render_fwd in FusedRender"] == T
    assert (n["PoseRays"], n["CamRays"]) == ((2 * T, 0) if opt_pose else (0, 2 * T))
