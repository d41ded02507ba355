"""Cross-view evaluation without a GPU: the CPU restatement ``tests/crossview_reference.py`` against the reference's fixture
(``tests/golden/crossview.npz``, ``gen_golden_crossview.py``), the host side (pair table, off-diagonal means, ``cross_eval.pth``), the ABI
entry and what the public functions refuse."""
import ctypes as C

import numpy as np
import pytest
import torch

import crossview_reference as CR
from oracle_bands import C_FP32

# what gen_golden_crossview.py printed: the largest distance of the restatement from the reference's recorded values over the 18 pairs,
# (rgb, depth_pred_vec, loss, depth error).  Scales: rgb 8.3e-2, depth 36.3, loss 1.36, depth error 3.54.
DIST_FP32 = dict(rgb=0.0, depth=0.0, mse_fg=0.0, depth_err=0.0)
DIST_F64 = dict(rgb=6.187e-08, depth=3.376e-06, mse_fg=1.152e-07, depth_err=3.195e-06)


@pytest.fixture(scope="module")
def amd():
    import supnerf_amd
    return supnerf_amd


@pytest.fixture(scope="module")
def fixture(golden):
    g = golden("crossview")
    return g, CR.fixture_views(g)


def distances(res, g):
    P = g["pairs"].shape[0]
    d = dict(rgb=0.0, depth=0.0, mse_fg=0.0, depth_err=0.0)
    for k in range(P):
        d["rgb"] = max(d["rgb"], float((res["rgb"][k].double() - g["rgb"][k].double()).abs().max()))
        d["depth"] = max(d["depth"], float((res["depth"][k].double() - g[f"depth_pred_vec{k}"].double()).abs().max()))
        d["mse_fg"] = max(d["mse_fg"], abs(float(res["mse_fg"][k]) - float(g["loss"][k])))
        d["depth_err"] = max(d["depth_err"], abs(float(res["depth_err"][k]) - float(g["depth_err"][k])))
    return d


def test_restatement_against_the_fixture(fixture, oracle_params):
    """The restatement on the recorded draws.  Targets and labels are the reference's, exactly.  Measured by the generator (above): the fp32
    restatement reproduced the reference's rgb, depths, loss and depth error BIT FOR BIT on the machine that made the fixture (distance 0
    in all four), the float64 restatement lies 6.2e-8 (rgb), 3.4e-6 (depth), 1.2e-7 (loss), 3.2e-6 (depth error) from them.  A band of
    4 x 0 would demand the generating machine's BLAS and thread count of every machine; the reference's OWN fp32 rounding error is its
    distance from the float64 evaluation, so the fp32 run is held within ``C_FP32`` = 4 times the larger of the two printed distances --
    another sample of the same rounding noise -- and the float64 run must be no further from the reference than that same band.  PSNR
    follows from the loss by the float64 formula, exactly."""
    g, views = fixture
    S, im_sz = int(g["n_samples"]), int(g["render_im_sz"])
    sc, tc = g["sc"].reshape(-1, 256), g["tc"].reshape(-1, 256)
    r32 = CR.evaluate(oracle_params, views, sc, tc, g["pairs"], g["jitter"], S, im_sz, torch.float32)
    r64 = CR.evaluate(oracle_params, views, sc, tc, g["pairs"], g["jitter"].double(), S, im_sz, torch.float64)
    for k in range(g["pairs"].shape[0]):
        assert torch.equal(r32["rgb_tgt"][k], g["rgb_tgt"][k]) and torch.equal(r32["occ"][k], g["occ_pixels"][k])
        assert r32["rgb"][k].dtype == torch.float32 and r64["rgb"][k].dtype == torch.float64
    d32, d64 = distances(r32, g), distances(r64, g)
    print("fp32", d32, "float64", d64)
    for key in d32:
        band = C_FP32 * max(DIST_FP32[key], DIST_F64[key])
        assert d32[key] <= band, (key, d32[key], band)
        assert d64[key] <= band, (key, d64[key], band)
    assert np.array_equal(g["dist_fp32"], np.array([DIST_FP32[k] for k in ("rgb", "depth", "mse_fg", "depth_err")]))
    # the reference's PSNR line on its own fp32 loss, and the restatement's on its own
    want = np.array([-10 * np.log(float(x)) / np.log(10) for x in g["loss"]])
    assert np.array_equal(np.asarray(g["psnr"]), want)
    assert np.array_equal(r32["psnr"], np.array([CR.psnr_of(x) for x in r32["mse_fg"]]))
    assert np.array_equal(np.asarray(g["psnr_mat"]).reshape(-1), np.asarray(g["psnr"])) and \
        np.array_equal(np.asarray(g["depth_mat"]).reshape(-1), np.asarray(g["depth_err"]))


def test_cross_pairs_table(amd):
    """View counts (3, 2), C = 2: instance-major, then snapshot, then ii, then num; code row = c V + ii over all V = 5 views."""
    pairs, off = amd.ops.cross_pairs(amd.ops.view_offset_of((3, 2)), 2)
    want = [[0, 0], [0, 1], [0, 2], [1, 0], [1, 1], [1, 2], [2, 0], [2, 1], [2, 2],
            [5, 0], [5, 1], [5, 2], [6, 0], [6, 1], [6, 2], [7, 0], [7, 1], [7, 2],
            [3, 3], [3, 4], [4, 3], [4, 4],
            [8, 3], [8, 4], [9, 3], [9, 4]]
    assert pairs.dtype == torch.int32 and pairs.tolist() == want and pairs.is_contiguous()
    assert off.dtype == torch.int64 and off.tolist() == [0, 18, 26]
    for bad in ((0, 3, 3), (1, 3), (0,)):
        with pytest.raises(amd.SnrError):
            amd.ops.cross_pairs(bad, 2)
    with pytest.raises(amd.SnrError):
        amd.ops.cross_pairs((0, 3), 0)


def test_cross_view_means_are_the_references(amd, fixture):
    """The off-diagonal means of the fixture's matrices: what the reference's ``collect_eval_results`` plotted from the file our writer made."""
    g, _ = fixture
    results = {0: (np.asarray(g["psnr_mat"]), np.asarray(g["depth_mat"]))}
    psnr, depth = amd.io.cross_view_means(results)
    assert np.array_equal(psnr, np.asarray(g["cross_psnr_mean"])) and np.array_equal(depth, np.asarray(g["cross_depth_mean"]))
    # an instance with one view adds nothing; two instances pool their entries
    m = np.arange(8, dtype=np.float64).reshape(2, 2, 2)
    both = amd.io.cross_view_means({0: (m, 2 * m), 1: (np.zeros((2, 1, 1)), np.zeros((2, 1, 1)))})
    assert both[0].tolist() == [1.5, 5.5] and both[1].tolist() == [3.0, 11.0]


def test_cross_eval_file_round_trip(amd, fixture, tmp_path):
    g, _ = fixture
    psnr, depth = np.asarray(g["psnr_mat"]), np.asarray(g["depth_mat"])
    path = amd.io.save_cross_eval(str(tmp_path), {0: (psnr, depth), 3: (psnr[:, :2, :2], depth[:, :2, :2])}, [0, 5], ids={0: "ins-a", 3: "ins-b"})
    assert path.endswith("cross_eval.pth")
    saved = torch.load(path, map_location="cpu", weights_only=False)
    assert sorted(saved) == ["CODE_SAVE_ITERS_", "cnt_lidar_pts_per_ins", "depth_eval_mat_per_ins", "psnr_eval_mat_per_ins"]
    assert saved["CODE_SAVE_ITERS_"] == [0, 5] and saved["cnt_lidar_pts_per_ins"] == {}
    assert list(saved["psnr_eval_mat_per_ins"]) == ["ins-a", "ins-b"] == list(saved["depth_eval_mat_per_ins"])
    for key, want in (("psnr_eval_mat_per_ins", psnr), ("depth_eval_mat_per_ins", depth)):
        mats = saved[key]["ins-a"]
        assert isinstance(mats, list) and len(mats) == 2
        for c, m in enumerate(mats):
            assert isinstance(m, np.ndarray) and m.dtype == np.float64 and m.shape == (3, 3) and np.array_equal(m, want[c])
        assert saved[key]["ins-b"][1].shape == (2, 2)
    means = amd.io.cross_view_means(saved)                                            # the loaded file is read like the driver's dict
    assert np.allclose(means[0], amd.io.cross_view_means({0: (psnr, depth), 3: (psnr[:, :2, :2], depth[:, :2, :2])})[0], rtol=0, atol=0)
    with pytest.raises(ValueError):
        amd.io.save_cross_eval(str(tmp_path), {0: (psnr, depth)}, [0, 5, 9])


def test_abi_entry(amd):
    assert amd._lib.header_abi_version() >= 20
    assert "snr_cross_metrics" in amd._lib.exported_symbols()
    lib = amd._lib.lib()
    assert lib.snr_abi_version() >= 20
    E_ARG = -1
    buf = (C.c_float * 64)()                                                          # never dereferenced: every call returns before a launch
    q = C.c_void_p(C.addressof(buf))
    host = (C.c_int32 * 4)(0, 0, 1, 1)

    def call(ptrs=None, P=2, V=2, n_codes=2, n=4, n_l=1, pairs_host=host):
        ptrs = ptrs or [q] * 8
        return lib.snr_cross_metrics(*ptrs[:7], pairs_host, P, V, n_codes, n, n_l, ptrs[7], None)
    for k in (0, 2, 3, 6, 7):                                                         # rgb, tgt, occ, pairs, out
        ptrs = [q] * 8
        ptrs[k] = None
        assert call(ptrs) == E_ARG
    for k in (1, 4, 5):                                                               # depth_pred, lid_depth, lid_cnt: needed when n_l > 0
        ptrs = [q] * 8
        ptrs[k] = None
        assert call(ptrs) == E_ARG
    assert call(n=0) == E_ARG and call(n_l=-1) == E_ARG and call(P=0) == E_ARG and call(V=0) == E_ARG
    assert call(pairs_host=(C.c_int32 * 4)(0, 0, 1, 2)) == E_ARG                      # target view 2 of V = 2
    assert call(pairs_host=(C.c_int32 * 4)(2, 0, 1, 1)) == E_ARG                      # code row 2 of 2
    assert call(pairs_host=(C.c_int32 * 4)(0, -1, 1, 1)) == E_ARG


def test_refusals(amd):
    ops, D = amd.ops, amd.driver
    P, V, n, n_l = 2, 2, 8, 3
    args = [torch.zeros(P, n, 3), torch.zeros(P, n_l), torch.zeros(V, n, 3), torch.zeros(V, n), torch.zeros(V, n_l),
            torch.zeros(V, dtype=torch.int32), torch.tensor([[0, 0], [1, 1]], dtype=torch.int32)]
    with pytest.raises(amd.SnrError):
        ops.cross_metrics(*args)                                                      # CPU tensors
    model = amd.CodeNeRF(3, 1)
    inst = D.make_instances([3], 2, lidar=True)
    hp = D.load_hpams()
    hp["n_samples"], hp["render_im_sz"] = 16, 8
    sc = torch.zeros(2, 256)
    with pytest.raises(amd.SnrError, match="GPU"):
        D.eval_cross_view(model, "cpu", inst, hp, sc, sc)
    with pytest.raises(amd.SnrError, match="sym_aug"):
        D.eval_cross_view(model, "cpu", inst, dict(hp, sym_aug=1), sc, sc)
    for bad in (torch.zeros(3, 256), torch.zeros(2, 128), torch.zeros(256), torch.zeros(1, 2, 2, 256), torch.zeros(0, 2, 256)):
        with pytest.raises(amd.SnrError, match="256"):
            D.eval_cross_view(model, "cpu", inst, hp, bad, bad)
    with pytest.raises(amd.SnrError, match="256"):
        D.eval_cross_view(model, "cpu", inst, hp, torch.zeros(2, 2, 256), sc)          # shape and texture snapshots disagree
    with pytest.raises(amd.SnrError):
        D.optimize_instances(model, "cpu", inst, hp, sc[:1], sc[:1], [1, 2], code_save_iters=[3, 2])
