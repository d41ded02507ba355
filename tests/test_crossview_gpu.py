"""Cross-view evaluation on the GPU: the kernel of csrc/snr_cross.hip against its float64 definition at its seams, ``driver.eval_cross_view``
against the CPU restatement ``tests/crossview_reference.py`` on the reference's fixture, against itself (batches, chunks, defective views)
and against the fit loop's own iteration-0 metrics, and the code snapshots the fit loops hand to it."""
import numpy as np
import pytest
import torch

import crossview_reference as CR
from conftest import load_golden
from oracle import supnerf_oracle as O
from oracle_bands import BANDS, amd, band_of, check_per_object, dev, in_band  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def make_model(amd, dev, precision):
    m = amd.CodeNeRF(3, 1)
    m.load_state_dict(O.init_decoder_params())
    m.precision = precision
    return m.to(dev)


@pytest.fixture(scope="module")
def model(amd, dev):
    return make_model(amd, dev, "fp32")


# ------------------------------------------------------------------------------------------------ the kernel
def kernel_case(seed, n, P, V, n_l, lid_cnt, pairs, zero_occ_view=None):
    g = torch.Generator().manual_seed(seed)
    rgb, tgt = torch.rand(P, n, 3, generator=g), torch.rand(V, n, 3, generator=g)
    occ = (torch.randint(0, 3, (V, n), generator=g) - 1).float()
    depth_pred, lid_depth = torch.rand(P, n_l, generator=g) * 30 + 5, torch.rand(V, n_l, generator=g) * 30 + 5
    if zero_occ_view is not None:
        occ[zero_occ_view] = 0
    return dict(rgb=rgb, depth_pred=depth_pred, tgt=tgt, occ=occ, lid_depth=lid_depth, lid_cnt=torch.tensor(lid_cnt, dtype=torch.int32),
                pairs=torch.tensor(pairs, dtype=torch.int32))


def run_kernel(amd, dev, case, name):
    args = [case[k] for k in ("rgb", "depth_pred", "tgt", "occ", "lid_depth", "lid_cnt")]
    got = amd.ops.cross_metrics(*[t.to(dev).contiguous() for t in args], case["pairs"]).cpu()
    o32, o64 = CR.metrics_definition(*args, case["pairs"], torch.float32), CR.metrics_definition(*args, case["pairs"], torch.float64)
    assert got.shape == (case["pairs"].shape[0], 3)
    for col, what in enumerate(("mse_fg", "depth_err", "sum_abs_occ")):
        ok, _, msg = in_band(got[:, col], o32[:, col], o64[:, col], "fp32", f"{name} {what}")
        print(msg)
        assert ok, msg
    return got


def test_kernel_fewer_rays_than_threads_and_repeated_views(amd, dev):
    """(a) n = 64 < 256 threads, P = 5 over V = 3: target view 2 three times, target 0 twice, code rows that differ from the target view,
    lidar counts 0, 3 and all 7; two runs give the same bits."""
    case = kernel_case(1, 64, 5, 3, 7, (0, 3, 7), [[0, 0], [1, 0], [4, 2], [2, 1], [5, 2]])
    a, b = run_kernel(amd, dev, case, "a"), run_kernel(amd, dev, case, "a again")
    assert torch.equal(a, b)
    assert float(a[0, 1]) == 0.0 and float(a[1, 1]) == 0.0 and bool((a[2:, 1] > 0).all())           # lid_cnt 0: 0 / 1e-8


def test_kernel_more_rays_than_one_pass(amd, dev):
    """(b) n = 324 = 256 + 68: every thread's second pass and a tail; n_l = 300 crosses a pass as well."""
    run_kernel(amd, dev, kernel_case(2, 324, 2, 2, 300, (300, 257), [[0, 1], [1, 0]]), "b")


def test_kernel_no_depth_rays(amd, dev):
    """(c) n_l = 0: the depth column is 0, the rest as ever."""
    got = run_kernel(amd, dev, kernel_case(3, 100, 1, 1, 0, (0,), [[0, 0]]), "c")
    assert float(got[0, 1]) == 0.0 and float(got[0, 0]) > 0


def test_kernel_view_without_labels(amd, dev):
    """(d) view 1's occ is all zero: its pairs have mse 0 and sum |occ| 0 exactly, every other pair is as without the defect, bit for bit,
    and nothing is non-finite."""
    pairs = [[0, 0], [1, 1], [2, 2], [3, 1], [4, 0]]
    base = run_kernel(amd, dev, kernel_case(4, 200, 5, 3, 6, (6, 2, 4), pairs), "d base")
    got = run_kernel(amd, dev, kernel_case(4, 200, 5, 3, 6, (6, 2, 4), pairs, zero_occ_view=1), "d")
    assert bool(torch.isfinite(got).all())
    assert bool((got[[1, 3], 0] == 0).all()) and bool((got[[1, 3], 2] == 0).all()) and torch.equal(got[[1, 3], 1], base[[1, 3], 1])
    assert torch.equal(got[[0, 2, 4]], base[[0, 2, 4]])


def test_host_pairs_are_refused_before_the_launch(amd, dev):
    case = kernel_case(5, 32, 2, 2, 3, (3, 3), [[0, 0], [1, 2]])                                       # target view 2 of V = 2
    args = [case[k].to(dev) for k in ("rgb", "depth_pred", "tgt", "occ", "lid_depth", "lid_cnt")]
    with pytest.raises(amd.SnrError):
        amd.ops.cross_metrics(*args, case["pairs"])
    with pytest.raises(amd.SnrError):
        amd.ops.cross_metrics(*args, torch.tensor([[0, 0], [3, 1]], dtype=torch.int32), n_codes=3)      # code row 3 of 3
    with pytest.raises(amd.SnrError):
        amd.ops.cross_metrics(args[0], args[1], args[2][:, :16], *args[3:], torch.tensor([[0, 0], [1, 1]], dtype=torch.int32))


# ------------------------------------------------------------------------------------------------ the driver on the reference's fixture
def hpams(D, S=16, im_sz=16, num_opts=1):
    hp = D.load_hpams()
    hp["n_samples"], hp["render_im_sz"], hp["optimize"]["num_opts"] = S, im_sz, num_opts
    return hp


@pytest.fixture(scope="module")
def fixture_case(oracle_params):
    """The fixture's inputs and the restatement of its 18 pairs in fp32 and float64, computed once."""
    g = load_golden("crossview")
    views = CR.fixture_views(g)
    S, im_sz = int(g["n_samples"]), int(g["render_im_sz"])
    sc, tc = g["sc"].reshape(-1, 256), g["tc"].reshape(-1, 256)
    o32 = CR.evaluate(oracle_params, views, sc, tc, g["pairs"], g["jitter"], S, im_sz, torch.float32)
    o64 = CR.evaluate(oracle_params, views, sc, tc, g["pairs"], g["jitter"].double(), S, im_sz, torch.float64)
    return g, views, o32, o64


@pytest.mark.parametrize("precision", ["fp32", "auto"])
def test_driver_against_the_restatement(amd, dev, fixture_case, precision):
    """The fixture's 2 snapshots x 3 x 3 pairs with the reference's draws: per pair, mse_fg and depth_err within the band of the arithmetic
    the launch ran in of the float64 restatement; the returned PSNR is the float64 formula of the returned fp32 mse."""
    g, views, o32, o64 = fixture_case
    D = amd.driver
    hp = hpams(D, int(g["n_samples"]), int(g["render_im_sz"]))
    info = {}
    res = D.eval_cross_view(make_model(amd, dev, precision), dev, [dict(views=views)], hp, g["sc"], g["tc"], jitter=g["jitter"], info=info)
    assert list(res) == [0] and info["skipped"] == [] and torch.equal(info["pairs"], g["pairs"])
    psnr, depth = res[0]
    assert psnr.shape == depth.shape == (2, 3, 3) and psnr.dtype == depth.dtype == np.float64
    m = info["metrics"]
    check_per_object([("mse_fg", m[:, 0], o32["mse_fg"], o64["mse_fg"]), ("depth_err", m[:, 1], o32["depth_err"], o64["depth_err"])],
                     band_of(precision))
    assert np.array_equal(psnr.reshape(-1), np.array([CR.psnr_of(x) for x in m[:, 0].tolist()]))
    assert np.array_equal(depth.reshape(-1), m[:, 1].numpy().astype(np.float64))


# ------------------------------------------------------------------------------------------------ the driver against itself
def lidar_instances(D, ids, counts):
    inst = []
    for i, n in zip(ids, counts):
        one = D.make_instances([i], n, lidar=True)[0]
        inst.append(one)
    return inst


def codes(C_, V, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(C_, V, 256, generator=g) * 0.3, torch.randn(C_, V, 256, generator=g) * 0.3


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_batch_and_chunk_independence(amd, dev, model):
    """Instances with 3, 2 and 1 views, C = 2: the one-view instance is skipped; every instance's matrices equal, bit for bit, a run on that
    instance alone (its pairs' launches read nothing of the others: every object of the fused forward has its own rows, and the lidar
    tables' padding -- to another width alone -- only adds rays whose depths the kernel never reads); one pair per launch equals one launch
    for all pairs."""
    D = amd.driver
    hp = hpams(D)
    inst = lidar_instances(D, [3, 8, 21], (3, 2, 1))
    sc, tc = codes(2, 6, 11)
    P = 2 * (9 + 4)
    jit = torch.rand(P, 2, 16, generator=torch.Generator().manual_seed(12))
    info = {}
    res = D.eval_cross_view(model, dev, inst, hp, sc, tc, jitter=jit, info=info)
    assert sorted(res) == [0, 1] and info["skipped"] == [2] and info["pair_offset"].tolist() == [0, 18, 26]
    assert res[0][0].shape == (2, 3, 3) and res[1][1].shape == (2, 2, 2)
    assert all(np.isfinite(x).all() for r in res.values() for x in r)
    alone0 = D.eval_cross_view(model, dev, inst[:1], hp, sc[:, :3], tc[:, :3], jitter=jit[:18])
    alone1 = D.eval_cross_view(model, dev, inst[1:2], hp, sc[:, 3:5], tc[:, 3:5], jitter=jit[18:])
    assert same(res[0], alone0[0]) and same(res[1], alone1[0])
    info1 = {}
    one = D.eval_cross_view(model, dev, inst, hp, sc, tc, jitter=jit, pair_chunk=1, info=info1)
    assert info1["pair_chunk"] == 1 and info["pair_chunk"] >= P
    assert same(res[0], one[0]) and same(res[1], one[1])
    # (V,256) codes are one snapshot: the second one's pairs are 9..17 of instance 0 and 22..25 of instance 1
    flat = D.eval_cross_view(model, dev, inst, hp, sc[1], tc[1], jitter=jit[list(range(9, 18)) + list(range(22, 26))])
    assert np.array_equal(flat[0][0][0], res[0][0][1]) and np.array_equal(flat[1][1][0], res[1][1][1])


def test_default_draws_are_seeded(amd, dev, model):
    """Without ``jitter`` every pair draws from its own CPU generator: seed base + p, or the listed seeds."""
    D = amd.driver
    hp = hpams(D)
    inst = lidar_instances(D, [4], (2,))
    sc, tc = codes(1, 2, 18)
    base = D.eval_cross_view(model, dev, inst, hp, sc, tc)[0]
    assert same(base, D.eval_cross_view(model, dev, inst, hp, sc, tc, seeds=[0, 1, 2, 3])[0])
    assert same(base, D.eval_cross_view(model, dev, inst, hp, sc, tc, jitter=torch.stack(
        [torch.rand(2, 16, generator=torch.Generator().manual_seed(p)) for p in range(4)]))[0])
    assert not same(base, D.eval_cross_view(model, dev, inst, hp, sc, tc, seeds=7)[0])
    with pytest.raises(amd.SnrError):
        D.eval_cross_view(model, dev, inst, hp, sc, tc, seeds=[0, 1, 2])
    with pytest.raises(amd.SnrError):
        D.eval_cross_view(model, dev, inst, hp, sc, tc, jitter=torch.zeros(4, 2, 8))
    with pytest.raises(amd.SnrError):
        D.eval_cross_view(model, dev, inst, hp, sc, tc, pair_chunk=0)


def test_defective_views(amd, dev, model):
    """A view with empty lidar lists: its depth column is 0; a view whose mask is all zero: its PSNR column is +inf.  Every pair that does
    not involve the view is as in the run without the defect, bit for bit."""
    D = amd.driver
    hp = hpams(D)
    inst = lidar_instances(D, [5], (3,))
    sc, tc = codes(1, 3, 13)
    jit = torch.rand(9, 2, 16, generator=torch.Generator().manual_seed(14))
    base = D.eval_cross_view(model, dev, inst, hp, sc, tc, jitter=jit)[0]

    def with_view(v, **change):
        views = [dict(x) for x in inst[0]["views"]]
        views[v].update(change)
        return D.eval_cross_view(model, dev, [dict(views=views)], hp, sc, tc, jitter=jit)[0]
    others = lambda m, v: np.delete(np.delete(m, v, 1), v, 2)
    psnr, depth = with_view(1, lidar_xy=np.zeros((0, 2), dtype=np.int64), lidar_depth=np.zeros(0, dtype=np.float32))
    assert (depth[:, :, 1] == 0).all() and (depth[:, :, [0, 2]] > 0).all()
    assert np.array_equal(psnr, base[0]) and np.array_equal(others(depth, 1), others(base[1], 1))
    psnr, depth = with_view(2, mask=torch.zeros_like(inst[0]["views"][2]["mask"]))
    assert np.isposinf(psnr[:, :, 2]).all() and np.isfinite(psnr[:, :, :2]).all() and np.isfinite(depth).all()
    assert np.array_equal(others(psnr, 2), others(base[0], 2)) and np.array_equal(depth, base[1])


def test_diagonal_is_the_loops_first_iteration(amd, dev, model, oracle_params):
    """``optimize_instances(opt_pose=False, sampling="grid")`` logs, in iteration 0, the PSNR and depth error of the start codes in every
    view's own camera: the diagonal of the cross-view matrices of the iteration-0 snapshot, fed the same draws.  The loop's PSNR averages
    over the foreground (occ > 0, src/optimizer_nuscenes.py:739-742), the cross-view one over |occ| (:1359-1360); they are the same number
    exactly when no label is -1, so the masks here are clamped to {0, 1}.  Both mse within the fp32 band of the float64 restatement, and
    the two PSNR within 4.35 dB times that relative band of each other (d(10 log10 x) = 4.34 dx / x)."""
    D = amd.driver
    hp = hpams(D, num_opts=1)
    inst = lidar_instances(D, [7], (3,))
    for view in inst[0]["views"]:
        view["mask"] = view["mask"].clamp_min(0)
        view["img"] = view["img"] * (view["mask"] > 0) + (view["mask"] <= 0)
    views = inst[0]["views"]
    g = torch.Generator().manual_seed(15)
    sc0, tc0 = torch.randn(1, 256, generator=g) * 0.3, torch.randn(1, 256, generator=g) * 0.3
    jit = torch.rand(1, 2, 3, 16, generator=g)
    info = {}
    metrics, *_ = D.optimize_instances(model, dev, inst, hp, sc0, tc0, [1, 2, 3], opt_pose=False, sampling="grid", jitter=jit, info=info,
                                       code_save_iters=[0])
    assert info["shape_snapshots"].shape == (1, 1, 256)
    off = tuple(info["view_offset"].tolist())
    sc_v = amd.ops.instance_rows_fwd(info["shape_snapshots"][0], off)
    tc_v = amd.ops.instance_rows_fwd(info["texture_snapshots"][0], off)
    pair_jit = torch.zeros(9, 2, 16)
    for v in range(3):
        pair_jit[4 * v] = jit[0, :, v]                                                                # pair (v, v) is row 3 v + v
    info_c = {}
    psnr, depth = D.eval_cross_view(model, dev, inst, hp, sc_v, tc_v, jitter=pair_jit, info=info_c)[0]
    diag = torch.tensor([0, 4, 8])
    pairs = info_c["pairs"][diag]
    o32 = CR.evaluate(oracle_params, views, sc0.expand(3, 256), tc0.expand(3, 256), pairs, pair_jit[diag], 16, 16, torch.float32)
    o64 = CR.evaluate(oracle_params, views, sc0.expand(3, 256), tc0.expand(3, 256), pairs, pair_jit[diag].double(), 16, 16, torch.float64)
    loop_psnr, loop_depth = metrics[:, 0, 0].cpu().double(), metrics[:, 0, 1].cpu().double()
    mse_cross, mse_loop = info_c["metrics"][diag, 0].double(), 10.0 ** (-loop_psnr / 10)
    c_, floor = BANDS["fp32"]
    for v in range(3):
        for name, got in (("cross", mse_cross[v]), ("loop", mse_loop[v])):
            ok, _, msg = in_band(got, o32["mse_fg"][v], o64["mse_fg"][v], "fp32", f"mse {name} view {v}")
            print(msg)
            assert ok, msg
        ok, _, msg = in_band(torch.tensor(depth[0, v, v]), o32["depth_err"][v], o64["depth_err"][v], "fp32", f"depth_err cross view {v}")
        assert ok, msg
        ok, _, msg = in_band(loop_depth[v], o32["depth_err"][v], o64["depth_err"][v], "fp32", f"depth_err loop view {v}")
        assert ok, msg
        rel_band = c_ * abs(float(o32["mse_fg"][v]) - float(o64["mse_fg"][v])) / float(o64["mse_fg"][v]) + floor
        print(f"view {v}: psnr cross {psnr[0, v, v]:.6f} loop {float(loop_psnr[v]):.6f}, allowed {4.35 * rel_band:.2e} dB")
        assert abs(psnr[0, v, v] - float(loop_psnr[v])) <= 4.35 * rel_band


# ------------------------------------------------------------------------------------------------ snapshots of the fit loops
def test_snapshots_of_the_instance_loop(amd, dev, model):
    """num_opts = 3, code_save_iters = [0, 1, 5]: row 0 the start codes, row 1 the codes a one-iteration run returns, row 2 (past the end)
    the returned codes -- all bit for bit; and ``code_save_iters=None`` is the loop as it was."""
    D = amd.driver
    inst = lidar_instances(D, [3, 8], (2, 1))
    g = torch.Generator().manual_seed(16)
    sc0, tc0 = torch.randn(2, 256, generator=g) * 0.3, torch.randn(2, 256, generator=g) * 0.3
    jit = torch.rand(3, 2, 3, 16, generator=g)
    seeds = [31, 32, 33]
    run = lambda T, **kw: D.optimize_instances(model, dev, inst, hpams(D, num_opts=T), sc0, tc0, seeds, opt_pose=False, sampling="grid",
                                               jitter=jit[:T], **kw)
    info = {}
    got = run(3, info=info, code_save_iters=[0, 1, 5])
    ss, ts = info["shape_snapshots"].cpu(), info["texture_snapshots"].cpu()
    assert ss.shape == ts.shape == (3, 2, 256)
    assert torch.equal(ss[0], sc0) and torch.equal(ts[0], tc0)
    one = run(1)
    assert torch.equal(ss[1], one[1].cpu()) and torch.equal(ts[1], one[2].cpu()) and not torch.equal(ss[1], ss[0])
    assert torch.equal(ss[2], got[1].cpu()) and torch.equal(ts[2], got[2].cpu()) and not torch.equal(ss[2], ss[1])
    plain, none = run(3), run(3, code_save_iters=None)
    for a, b, c in zip(got, plain, none):
        assert torch.equal(a, b) and torch.equal(b, c)
    with pytest.raises(amd.SnrError):
        run(3, code_save_iters=[1, 1])


def test_snapshots_of_the_batched_loop(amd, dev, model):
    """``optimize_objects_batched`` with render-only iterations (reg_iters = 0: no step after iteration 0): the snapshot entering
    iteration 1 still holds the start codes, the one entering iteration 2 has moved, the one past the end is what the loop returns."""
    D = amd.driver
    objs = D.make_objects([3, 8], 16, lidar=True)
    g = torch.Generator().manual_seed(17)
    sc0, tc0 = torch.randn(2, 256, generator=g) * 0.3, torch.randn(2, 256, generator=g) * 0.3
    jit = torch.rand(3, 2, 2, 16, generator=g)
    info = {}
    got = D.optimize_objects_batched(model, dev, objs, hpams(D, num_opts=3), sc0, tc0, [41, 42], reg_iters=0, jitter=jit, info=info,
                                     code_save_iters=[0, 1, 2, 3])
    ss = info["shape_snapshots"].cpu()
    assert ss.shape == (4, 2, 256) and torch.equal(ss[0], sc0) and torch.equal(ss[1], sc0) and not torch.equal(ss[2], sc0)
    assert torch.equal(ss[3], got[1].cpu()) and torch.equal(info["texture_snapshots"][3].cpu(), got[2].cpu())
    plain = D.optimize_objects_batched(model, dev, objs, hpams(D, num_opts=3), sc0, tc0, [41, 42], reg_iters=0, jitter=jit)
    for a, b in zip(got, plain):
        assert torch.equal(a, b)
