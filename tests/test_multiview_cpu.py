"""Multi-view fit, host side (no GPU): the restatement ``tests/multiview_reference.py`` against the fixture recorded from the reference
(``tests/golden/multiview.npz``, ``gen_golden_multiview.py``), the properties the device loop leans on (the shared codes' gradient is the
sum of the views' gradients; a ray with occupancy 0 weighs nothing in the loss), the view <-> instance layout, the C ABI's argument checks
(no launch is made) and the driver's argument errors."""
import ctypes as C

import numpy as np
import pytest
import torch

import multiview_reference as MR
from cpu_arith import golden_tol
from oracle import supnerf_oracle as O
from oracle_bands import amd  # noqa: F401  (a fixture)


def same(a, b, tol=0.0):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= golden_tol(b, tol), (float((a - b).abs().max()), tol)


def fixture_views(g):
    return [dict(img=g[f"img{v}"], mask=g[f"mask{v}"], cam_pose=g[f"cam_pose{v}"], K=g[f"K{v}"], roi=g[f"roi{v}"], obj_diag=np.float32(g[f"obj_diag{v}"]))
            for v in range(2)]


def fixture_hpams(g, num_opts):
    lr = [float(v) for v in g["lr"]]
    return dict(n_samples=int(g["n_samples"]), render_im_sz=8, shapenet_obj_cood=1, loss_occ_coef=float(g["loss_occ_coef"]),
                optimize=dict(num_opts=num_opts, lr_shape=lr[0], lr_texture=lr[1], lr_pose=lr[2], lr_half_interval=1000, opt_cam_pose=0))


def test_restatement_reproduces_the_reference_fixture(golden, oracle_params):
    """2 views x 2 iterations of the reference's own render_rays / loss / AdamW: picks and gathered targets exactly; rendered values,
    accumulated gradients and stepped codes within the tolerances tests/test_oracle_golden.py gives its render_a_* (2e-6) and gradient
    (codes 1e-7, pose 1e-6) fixtures."""
    g = golden("multiview")
    views = fixture_views(g)
    T, V, n = g["picks"].shape
    assert (V, n) == (2, int(g["n_rays"])) and [int(v["img"].shape[0] * v["img"].shape[1]) for v in views] == [30, 63]
    rot0, tr0, _ = MR.start_poses(views, g["seeds"].tolist(), tuple(g["pose_noise"].tolist()), O.matrix_to_rotvec)
    same(rot0, g["rot0"], 4e-7); same(tr0, g["tr0"], 4e-6)                                   # (one float32 ulp of pi and of a 33 m translation)
    got = MR.fit(oracle_params, views, fixture_hpams(g, T), g["sc0"], g["tc0"], g["seeds"].tolist(), g["jitter"], picks=g["picks"].numpy(),
                 pose_noise=tuple(g["pose_noise"].tolist()), start=(g["rot0"], g["tr0"]))
    for it in range(T):
        for v in range(V):
            rgb, acc, tgt, occ = got["renders"][it][v]
            ids = g["picks"][it, v].long()
            assert bool((ids >= 0).all()) and len(set(ids.tolist())) == n                    # a permutation's head: no pixel twice
            assert torch.equal(tgt, views[v]["img"].reshape(-1, 3)[ids]) and torch.equal(tgt, g["tgt"][it, v])      # picks and targets: exactly
            assert torch.equal(occ[:, 0], g["occ"][it, v])
            same(rgb, g["rgb"][it, v], 2e-6); same(acc, g["acc"][it, v], 2e-6)
            same(got["loss"][it, v], g["loss"][it, v], 1e-6)
        d_sc, d_tc, d_rot, d_tr = got["grads"][it]
        same(d_sc, g["g_sc"][it], 1e-7); same(d_tc, g["g_tc"][it], 1e-7); same(d_rot, g["g_rot"][it], 1e-6); same(d_tr, g["g_tr"][it], 1e-6)
        same(got["codes"][it][0], g["sc"][it], 1e-6); same(got["codes"][it][1], g["tc"][it], 1e-6)
    assert float((g["sc"][1] - g["sc"][0]).abs().max()) > 1e-3                               # the second step moved the codes again


def test_shared_code_gradient_is_the_sum_of_the_views_gradients(golden, oracle_params):
    """float64: what accumulates in the shared codes over V backward calls is the sum of the V single-view gradients."""
    g = golden("multiview")
    views = fixture_views(g)
    hp = fixture_hpams(g, 1)
    seeds, noise = g["seeds"].tolist(), tuple(g["pose_noise"].tolist())
    kw = dict(pose_noise=noise, dtype=torch.float64, steps=False)
    both = MR.fit(oracle_params, views, hp, g["sc0"], g["tc0"], seeds, g["jitter"][:1], picks=g["picks"][:1].numpy(), **kw)
    singles = [MR.fit(oracle_params, [views[v]], hp, g["sc0"], g["tc0"], [seeds[v]], g["jitter"][:1, :, v:v + 1], picks=g["picks"][:1, v:v + 1].numpy(), **kw)
               for v in range(2)]
    for k in (0, 1):
        want = singles[0]["grads"][0][k] + singles[1]["grads"][0][k]
        got = both["grads"][0][k]
        assert float(want.abs().max()) > 1e-5
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    for v in (0, 1):                                                                         # and every view keeps its own pose gradient
        assert torch.equal(both["grads"][0][2][v], singles[v]["grads"][0][2][0])


def _padded(rgb, acc, tgt, occ, k, g):
    return (torch.cat([rgb, torch.rand(k, 3, generator=g).to(rgb.dtype)]), torch.cat([acc, torch.rand(k, generator=g).to(acc.dtype)]),
            torch.cat([tgt, torch.zeros(k, 3, dtype=tgt.dtype)]), torch.cat([occ, torch.zeros(k, 1, dtype=occ.dtype)]))


@pytest.mark.parametrize("n,k", [(42, 6), (63, 1), (30, 100)])
def test_rays_with_occupancy_zero_are_neutral_in_the_loss(n, k):
    """Appending rays with occ = 0 (whatever they render) leaves ``optimise_losses`` unchanged.

    Exactly: every appended term of every numerator and denominator is +0.0 and the first n terms keep their bits -- checked term by term --
    and with inputs whose partial sums are all exact in float32 (colours on a 1/16 grid, acc = 1/2 in the view's own rows, so exp() = 1) the
    four outputs are the same bits, whatever order ``torch.sum`` adds in.  With generic inputs the terms are still the same bits, but
    ``torch.sum`` on the CPU adds in blocks whose boundaries move with the length, so the SUMS may round differently by an ulp or two
    (measured here: 3e-8 on loss_rgb, 5e-7 on a PSNR of ~5 dB): there the outputs are held to 4 float32 ulps."""
    g = torch.Generator().manual_seed(100 * n + k)
    occ = (torch.randint(0, 3, (n, 1), generator=g) - 1).float()
    # (a) partial sums exact: the same bits
    rgb, tgt = torch.randint(0, 17, (n, 3), generator=g) / 16.0, torch.randint(0, 17, (n, 3), generator=g) / 16.0
    acc = torch.full((n,), 0.5)
    a = O.optimise_losses(rgb, acc, tgt, occ, 0.1)
    b = O.optimise_losses(*_padded(rgb, acc, tgt, occ, k, g), 0.1)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), [float(x - y) for x, y in zip(a, b)]
    # (b) generic inputs: the same terms, zeros appended
    rgb, tgt, acc = torch.rand(n, 3, generator=g), torch.rand(n, 3, generator=g), torch.rand(n, generator=g)
    rgb2, acc2, tgt2, occ2 = _padded(rgb, acc, tgt, occ, k, g)
    terms = lambda r, a_, t, o: (((r - t) ** 2) * o.abs(), torch.exp(-o * (0.5 - a_.unsqueeze(-1))) * o.abs(), ((r - t) ** 2) * o.clamp_min(0), o.abs())
    for x, y in zip(terms(rgb, acc, tgt, occ), terms(rgb2, acc2, tgt2, occ2)):
        assert torch.equal(y[:n], x) and bool((y[n:] == 0).all()) and not bool(torch.signbit(y[n:]).any())
    a, b = O.optimise_losses(rgb, acc, tgt, occ, 0.1), O.optimise_losses(rgb2, acc2, tgt2, occ2, 0.1)
    for x, y in zip(a, b):
        assert abs(float(x - y)) <= 4 * float(np.finfo(np.float32).eps) * max(1.0, abs(float(x)))


# ------------------------------------------------------------------------------------------------ layout, C ABI, driver arguments
def test_view_offsets(amd):
    assert amd.ops.view_offset_of([1, 4, 2]) == (0, 1, 5, 7) and amd.ops.view_offset_of([3]) == (0, 3)
    for bad in ([], [2, 0, 1], [-1]):
        with pytest.raises(amd.SnrError):
            amd.ops.view_offset_of(bad)
    D = amd.driver
    inst = D.make_instances([4, 9], 3)
    views, off = D._flatten_instances(inst)
    assert off == (0, 3, 6) and [v["index"] for v in views] == [4, 4, 4, 9, 9, 9] and [v["view"] for v in views] == [0, 1, 2, 0, 1, 2]
    sizes = {tuple(v["img"].shape[:2]) for v in views}
    assert len(sizes) > 1                                                                    # native rois: different sizes in one launch
    for i in inst:
        assert len({float(v["obj_diag"]) for v in i["views"]}) == 1                          # one car, one size
        for v in i["views"]:
            x0, y0, x1, y1 = [int(t) for t in v["roi"]]
            assert tuple(v["img"].shape) == (y1 - y0, x1 - x0, 3) and tuple(v["mask"].shape) == (y1 - y0, x1 - x0, 1)
            assert bool((v["img"][v["mask"][..., 0] <= 0] == 1).all())                       # background whitened
    picks = D.draw_view_picks(views[:2] + [dict(roi=torch.tensor([3, 4, 9, 11]))], [1, 2, 3], 3, 48)
    assert picks.shape == (3, 3, 48) and picks.dtype == torch.int32
    assert bool((picks[:, 2, 42:] == -1).all()) and sorted(picks[1, 2, :42].tolist()) == list(range(42))       # 6 x 7 pixels: all of them, then -1
    assert len(set(picks[0, 0].tolist())) == 48 and not torch.equal(picks[0, 0], picks[1, 0])


def test_abi_version_symbols_and_argument_checks(amd):
    assert amd._lib.header_abi_version() >= 19
    lib = amd._lib.lib()
    assert lib.snr_abi_version() == amd._lib.header_abi_version()
    for name in ("snr_view_pixels", "snr_instance_rows_fwd", "snr_instance_rows_bwd"):
        assert name in amd._lib.exported_symbols()
    host = lambda l: (C.c_int64 * len(l))(*l)
    one = C.c_void_p(8)                                                                      # a non-null address nothing reads: every case returns first
    for fn in (lib.snr_instance_rows_fwd, lib.snr_instance_rows_bwd):
        assert fn(one, one, host([0, 1, 1, 3]), 3, 3, 256, one, None) == -1                  # an instance without a view
        assert fn(one, one, host([0, 2, 1, 3]), 3, 3, 256, one, None) == -1                  # not ascending
        assert fn(one, one, host([0, 1, 2]), 2, 3, 256, one, None) == -1                     # does not end at V
        assert fn(one, one, host([1, 2, 3]), 2, 3, 256, one, None) == -1                     # does not start at 0
        assert fn(one, one, None, 3, 2, 256, one, None) == -1                                # fewer views than instances
        assert fn(one, one, host([0, 1]), 1, 1, 0, one, None) == -1                          # no column
        assert fn(one, one, None, 0, 0, 256, one, None) == -1
        assert fn(one, None, host([0, 1]), 1, 1, 256, one, None) == -1                       # null device offsets
        assert fn(None, one, host([0, 1]), 1, 1, 256, one, None) == -1
    args = [one] * 6
    assert lib.snr_view_pixels(*args, 0, 5, one, one, one, None) == 0 and lib.snr_view_pixels(*args, 5, 0, one, one, one, None) == 0
    assert lib.snr_view_pixels(*args, -1, 5, one, one, one, None) == -1 and lib.snr_view_pixels(*args, 2, -5, one, one, one, None) == -1
    for hole in range(6):
        a = list(args); a[hole] = None
        assert lib.snr_view_pixels(*a, 2, 5, one, one, one, None) == -1
    assert lib.snr_view_pixels(*args, 2, 5, None, one, one, None) == -1
    assert lib.snr_view_pixels(*args, 1 << 30, 1 << 30, one, one, one, None) == -5


def test_operators_refuse_cpu_tensors_and_bad_layouts(amd):
    ops = amd.ops
    with pytest.raises(amd.SnrError):
        ops.InstanceRows.apply(torch.zeros(2, 4, 256), (0, 1, 3))                            # no CPU path
    with pytest.raises(amd.SnrError):
        ops.view_pixels(torch.zeros(4, 3), torch.zeros(4), torch.tensor([0, 4]), torch.zeros(1, 4, dtype=torch.int32), torch.ones(1, 4),
                        torch.zeros(1, 2, dtype=torch.int32))
    import types
    assert ops.InstanceRows.backward(types.SimpleNamespace(), None) == (None, None)          # an output nobody differentiated: no launch
    for off in ((0, 1, 1), (0, 2), (1, 2, 3), (0, 2, 1)):
        with pytest.raises(amd.SnrError):
            ops._view_offset_args(off, 2, torch.device("cpu"))


def test_driver_argument_errors(amd, oracle_params):
    D = amd.driver
    model = amd.CodeNeRF(3, 1); model.load_state_dict(oracle_params)
    hp = D.load_hpams(); hp["optimize"]["num_opts"] = 2
    inst = D.make_instances([1], 2)
    codes = torch.zeros(1, 256)
    call = lambda instances, hp_=hp, seeds=(0, 1), **kw: D.optimize_instances(model, "cuda:0", instances, hp_, codes, codes, list(seeds), n_rays=16, **kw)
    with pytest.raises(amd.SnrError, match="no view"):
        call([dict(views=[])])
    with pytest.raises(amd.SnrError, match="no instance"):
        call([])
    with pytest.raises(amd.SnrError, match="sym_aug"):
        call(inst, dict(hp, sym_aug=1))
    with pytest.raises(amd.SnrError, match="slack_tex"):
        call(inst, dict(hp, slack_tex=1))
    with pytest.raises(amd.SnrError, match="opt_model"):
        call(inst, dict(hp, optimize=dict(hp["optimize"], opt_model=1)))
    with pytest.raises(amd.SnrError, match="one seed per view"):
        call(inst, seeds=(0,))
    with pytest.raises(amd.SnrError, match="sampling"):
        call(inst, sampling="stratified")
    half = D.make_instances([1], 2, lidar=True)
    half[0]["views"][1].pop("lidar_xy"); half[0]["views"][1].pop("lidar_depth")
    with pytest.raises(amd.SnrError, match="lidar"):
        call(half)
    with pytest.raises(amd.SnrError, match=r"\(I,256\)"):
        D.optimize_instances(model, "cuda:0", inst, hp, torch.zeros(2, 256), torch.zeros(2, 256), [0, 1], n_rays=16)
