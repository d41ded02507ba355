"""Multi-view fit on the GPU: the two kernels of csrc/snr_views.hip bit for bit against their definitions, and ``driver.optimize_instances``
against the batched single-view loop (same bits at one view per instance), the CPU restatement ``tests/multiview_reference.py`` (traces,
shared-code gradient in float64), itself (padding rays are neutral, runs are bit reproducible, a ragged batch equals its instances alone)."""
import ctypes as C

import numpy as np
import pytest
import torch

import multiview_reference as MR
from oracle import supnerf_oracle as O
from oracle_bands import amd, dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

FILL = -7.5                                        # sentinel around buffers handed to the C ABI
GUARD = 64


@pytest.fixture(scope="module")
def model(amd, dev):
    m = amd.CodeNeRF(3, 1)
    m.load_state_dict(O.init_decoder_params())
    m.precision = "fp32"
    return m.to(dev)


# ------------------------------------------------------------------------------------------------ view_pixels
def crops(rois, seed):
    g = torch.Generator().manual_seed(seed)
    img, occ, off = [], [], [0]
    for x0, y0, x1, y1 in rois:
        n = (x1 - x0) * (y1 - y0)
        img.append(torch.rand(n, 3, generator=g)); occ.append((torch.randint(0, 3, (n,), generator=g) - 1).float())
        off.append(off[-1] + n)
    return torch.cat(img), torch.cat(occ), torch.tensor(off, dtype=torch.int64)


def expected_view_pixels(img, occ, off, rois, Ks, picks):
    """The definition on the CPU: the torch expression of the loops' direction tables, plain gathers, padding rows (0,0,1) / 0 / 0."""
    V, n = picks.shape
    cam, tgt, oc = torch.zeros(V, n, 3), torch.zeros(V, n, 3), torch.zeros(V, n)
    cam[:, :, 2] = 1
    for v, (x0, y0, x1, y1) in enumerate(rois):
        w, h = x1 - x0, y1 - y0
        K = Ks[v]
        cx, cy, fx, fy = K[0, 2], K[1, 2], K[0, 0], K[1, 1]
        ids = picks[v].long()
        ok = (ids >= 0) & (ids < w * h)
        px, py = (x0 + ids[ok] % w).float(), (y0 + ids[ok] // w).float()
        cam[v, ok] = torch.stack([(px - cx) / fx, (py - cy) / fy, torch.ones_like(px)], -1)
        tgt[v, ok] = img[off[v] + ids[ok]]
        oc[v, ok] = occ[off[v] + ids[ok]]
    return cam, tgt, oc


def run_view_pixels(amd, dev, rois, Ks, picks, seed):
    img, occ, off = crops(rois, seed)
    want = expected_view_pixels(img, occ, off, rois, Ks, picks)
    f = lambda t: t.to(dev).contiguous()
    roi_d = f(torch.tensor(rois, dtype=torch.int32))
    Kvec = f(torch.stack([torch.stack([K[0, 0], K[1, 1], K[0, 2], K[1, 2]]) for K in Ks]))
    img_d, occ_d, off_d, picks_d = f(img), f(occ), f(off), f(picks)
    got = amd.ops.view_pixels(img_d, occ_d, off_d, roi_d, Kvec, picks_d)
    for a, b in zip(got, want):
        assert torch.equal(a.cpu(), b), float((a.cpu() - b).abs().max())
    # the same launch through the C ABI into the interiors of sentinel-filled buffers: the same bits, nothing outside them
    V, n = picks.shape
    bufs = [torch.full((GUARD + V * n * k + GUARD,), FILL, device=dev) for k in (3, 3, 1)]
    ptr = lambda t: C.c_void_p(t.data_ptr() + 4 * GUARD)
    rc = amd._lib.lib().snr_view_pixels(C.c_void_p(img_d.data_ptr()), C.c_void_p(occ_d.data_ptr()), C.c_void_p(off_d.data_ptr()),
                                        C.c_void_p(roi_d.data_ptr()), C.c_void_p(Kvec.data_ptr()), C.c_void_p(picks_d.data_ptr()), V, n,
                                        ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]), None)
    assert rc == 0
    torch.cuda.synchronize()
    for b, w in zip(bufs, want):
        b = b.cpu()
        assert torch.equal(b[GUARD:-GUARD], w.reshape(-1))
        assert bool((b[:GUARD] == FILL).all()) and bool((b[-GUARD:] == FILL).all())
    return want


def make_K(fx, fy, cx, cy):
    return torch.tensor([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def test_view_pixels_ragged_views_and_padding(amd, dev):
    """case A: V = 3, rois 5 x 7, 16 x 9 and 1 x 1 at non-zero origins, a K per view, n = 40: two views have fewer pixels than n."""
    rois = [(13, 7, 18, 14), (401, 250, 417, 259), (3, 899, 4, 900)]
    Ks = [make_K(1266.4, 1266.4, 816.3, 491.5), make_K(721.5, 733.25, 609.6, 172.9), make_K(2055.6, 2049.1, 939.7, 641.1)]
    n = 40
    picks = torch.full((3, n), -1, dtype=torch.int32)
    g = torch.Generator().manual_seed(3)
    for v, (x0, y0, x1, y1) in enumerate(rois):
        hw = (x1 - x0) * (y1 - y0)
        body = torch.randint(0, hw, (n - 8,), generator=g, dtype=torch.int32)
        # first and last pixel, a duplicate pair, -1, one index equal to h w, one far beyond, one very negative
        picks[v] = torch.cat([torch.tensor([0, hw - 1, body[0], body[0], -1, hw, hw + 1000, -2 ** 31], dtype=torch.int32), body])[torch.randperm(n, generator=g)]
    cam, tgt, occ = run_view_pixels(amd, dev, rois, Ks, picks, seed=1)
    pad = (picks < 0) | (picks >= torch.tensor([35, 144, 1])[:, None])
    assert int(pad.sum()) >= 3 * 4 and bool((cam[pad] == torch.tensor([0.0, 0.0, 1.0])).all()) and bool((tgt[pad] == 0).all()) and bool((occ[pad] == 0).all())
    assert bool((cam[~pad][:, :2] != 0).any())


def test_view_pixels_more_rays_than_a_block(amd, dev):
    """case B: V = 2, n = 300 crosses a 256-thread block."""
    rois = [(100, 50, 131, 73), (7, 9, 20, 40)]
    Ks = [make_K(1266.4, 1266.4, 816.3, 491.5), make_K(1000.0, 990.0, 12.5, 30.25)]
    g = torch.Generator().manual_seed(4)
    picks = torch.stack([torch.randint(-1, (x1 - x0) * (y1 - y0) + 1, (300,), generator=g, dtype=torch.int32) for x0, y0, x1, y1 in rois])
    run_view_pixels(amd, dev, rois, Ks, picks, seed=2)


def test_view_pixels_strided_threads(amd, dev):
    """more rays than the launch has threads (1024 blocks of 256): every thread takes a second ray"""
    rois = [(100, 50, 131, 73), (7, 9, 20, 40)]
    Ks = [make_K(1266.4, 1266.4, 816.3, 491.5), make_K(1000.0, 990.0, 12.5, 30.25)]
    n = 1024 * 256 // 2 + 777
    g = torch.Generator().manual_seed(5)
    picks = torch.stack([torch.randint(-1, (x1 - x0) * (y1 - y0) + 1, (n,), generator=g, dtype=torch.int32) for x0, y0, x1, y1 in rois])
    run_view_pixels(amd, dev, rois, Ks, picks, seed=3)


# ------------------------------------------------------------------------------------------------ instance rows
@pytest.mark.parametrize("n_lat", [4, 1])
def test_instance_rows(amd, dev, n_lat):
    """I = 3 with view counts (1, 4, 2), C = n_lat 256: forward = index_select; backward = the views added in ascending order, in fp32,
    with gradient values whose sum depends on the order."""
    counts, C_ = (1, 4, 2), n_lat * 256
    off = amd.ops.view_offset_of(counts)
    inst_of = torch.repeat_interleave(torch.arange(3), torch.tensor(counts))
    g = torch.Generator().manual_seed(6)
    rows = torch.randn(3, n_lat, 256, generator=g)
    rows_d = rows.to(dev).requires_grad_()
    out = amd.ops.InstanceRows.apply(rows_d, off)
    assert out.shape == (7, n_lat, 256) and torch.equal(out.detach().cpu(), rows.index_select(0, inst_of))
    d_out = torch.randn(7, C_, generator=g)
    d_out[1:5, :64] = torch.tensor([1e8, 1.0, -1e8, 1.0])[:, None]                 # ascending: ((1e8 + 1) - 1e8) + 1 = 1; descending: 0
    d_out[5:7, :8] = torch.tensor([3e7, 1.0])[:, None]

    def ordered(order):
        acc = torch.zeros(3, C_)
        for i in range(3):
            vs = list(range(off[i], off[i + 1]))[::order]
            acc[i] = d_out[vs[0]]
            for v in vs[1:]:
                acc[i] = acc[i] + d_out[v]
        return acc
    want, reverse = ordered(1), ordered(-1)
    assert not torch.equal(want, reverse) and float(want[1, 0]) == 1.0 and float(reverse[1, 0]) == 0.0     # the check has teeth
    runs = []
    for _ in range(2):
        rows_d.grad = None
        out = amd.ops.InstanceRows.apply(rows_d, off)
        out.backward(d_out.view(7, n_lat, 256).to(dev))
        runs.append(rows_d.grad.cpu().clone())
    assert torch.equal(runs[0].view(3, C_), want) and torch.equal(runs[0], runs[1])
    with pytest.raises(amd.SnrError):
        amd.ops.InstanceRows.apply(rows_d, (0, 1, 1, 7))                            # an instance without a view
    with pytest.raises(amd.SnrError):
        amd.ops.InstanceRows.apply(rows_d, (0, 1, 5))                               # offsets of another instance count


# ------------------------------------------------------------------------------------------------ the loop
def hpams(D, S=16, num_opts=6, im_sz=16):
    hp = D.load_hpams()
    hp["n_samples"], hp["render_im_sz"], hp["optimize"]["num_opts"] = S, im_sz, num_opts
    return hp


def small_view(amd, view, w, h, index):
    """A copy of ``view`` with a hand-made w x h roi about its centre and a native crop of that size."""
    x0, y0, x1, y1 = [int(t) for t in view["roi"]]
    cx, cy = (x0 + x1) // 2, (y0 + y1) // 2
    img, mask = amd.synthetic.synthetic_crop_targets(index, h, w)
    out = dict(view)
    out.update(roi=torch.tensor([cx - w // 2, cy - h // 2, cx - w // 2 + w, cy - h // 2 + h], dtype=torch.int32), img=img * (mask > 0) + (mask <= 0), mask=mask)
    return out


def start_codes(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 256, generator=g) * 0.3, torch.randn(n, 256, generator=g) * 0.3


def test_one_view_per_instance_is_the_batched_loop(amd, dev, model):
    """I = 3, one view each, the resized grid: the launches and their inputs are those of ``optimize_objects_batched`` stepping from
    iteration 0; a one-view expand is a copy and a one-term sum is that term -- identical bits in metrics, codes and poses."""
    D = amd.driver
    hp = hpams(D)
    inst = D.make_instances([3, 8, 21], 1)
    objs = [i["views"][0] for i in inst]
    sc0, tc0 = start_codes(3, 2)
    jit = torch.rand(6, 2, 3, 16, generator=torch.Generator().manual_seed(9))
    seeds = [103, 108, 121]
    info = {}
    got = D.optimize_instances(model, dev, inst, hp, sc0, tc0, seeds, opt_pose=True, sampling="grid", jitter=jit, info=info)
    want = D.optimize_objects_batched(model, dev, objs, hp, sc0, tc0, seeds, reg_iters=-1, jitter=jit)
    assert got[0].shape == (3, 6, 4) and info["view_offset"].tolist() == [0, 1, 2, 3] and info["rays_per_view"].tolist() == [256] * 3
    for a, b in zip(got, want):
        assert torch.equal(a.cpu(), b.cpu()), float((a.cpu() - b.cpu()).abs().max())


def check_traces(m, ref, first_exact=True):
    """The bands of tests/test_driver_gpu.py's single-view loop: identical until the first optimiser step, then fp32 drift amplified by
    Adam's normalisation."""
    ps, rot, tr = m[:, :, 0].cpu().T.double(), m[:, :, 2].cpu().T.double(), m[:, :, 3].cpu().T.double()
    d = (ps - ref["psnr"].double()).abs()
    print("psnr |gpu - restatement| per iteration:", d.max(dim=1).values.tolist())
    print("rot / trans error |gpu - restatement|:", float((rot - ref["rot_err"].double()).abs().max()), float((tr - ref["trans_err"].double()).abs().max()))
    if first_exact:
        assert float(d[0].max()) < 1e-3
    assert float(d.max()) < 0.05
    assert float((rot - ref["rot_err"].double()).abs().max()) < 2e-3 and float((tr - ref["trans_err"].double()).abs().max()) < 2e-3


def test_random_sampling_against_the_restatement(amd, dev, model):
    """I = 1, V = 2, random native pixels with given picks and jitter (n_rays 48; one view has a 6 x 7 roi, so 6 of its rays are padding)
    against the fp32 restatement on the CPU."""
    D = amd.driver
    hp = hpams(D)
    inst = D.make_instances([5], 2)
    inst[0]["views"][1] = small_view(amd, inst[0]["views"][1], 6, 7, 77)
    views = inst[0]["views"]
    sc0, tc0 = start_codes(1, 3)
    seeds = [31, 32]
    picks = D.draw_view_picks(views, [7, 8], 6, 48)
    assert bool((picks[:, 1, 42:] == -1).all()) and bool((picks[:, 0] >= 0).all())
    jit = torch.rand(6, 2, 2, 16, generator=torch.Generator().manual_seed(10))
    info = {}
    m, sc, tc, pose = D.optimize_instances(model, dev, inst, hp, sc0, tc0, seeds, n_rays=48, picks=picks, jitter=jit, info=info)
    assert info["rays_per_view"].tolist() == [48, 42] and m.shape == (2, 6, 4) and bool(torch.isfinite(m).all())
    ref = MR.fit(O.init_decoder_params(), views, hp, sc0, tc0, seeds, jit, picks=picks.numpy(), to_matrix=D.axis_angle_to_matrix,
                 to_vec=D.matrix_to_axis_angle)
    check_traces(m, ref)
    assert float((info["loss"].cpu().double() - ref["loss"].double()).abs()[0].max()) < 1e-5
    print("mean PSNR over the views, first and last iteration:", float(m[:, 0, 0].mean()), float(m[:, -1, 0].mean()))
    assert float(m[:, -1, 0].mean()) > float(m[:, 0, 0].mean())


def test_shared_code_gradient_against_float64(amd, dev, model, monkeypatch):
    """I = 1, V = 3, one iteration: the gradient the AdamW step reads from the shared codes against the float64 restatement.

    Bound: the relative error (largest entry error over the largest entry) may not exceed V times the largest relative error the three
    SINGLE-view gradients of the existing ``optimize_objects_batched`` path show against the same oracle: the errors of the summands add.
    Both numbers are printed."""
    D = amd.driver
    hp = hpams(D, num_opts=1)
    inst = D.make_instances([12], 3)
    views = inst[0]["views"]
    sc0, tc0 = start_codes(1, 4)
    seeds = [41, 42, 43]
    jit = torch.rand(1, 2, 3, 16, generator=torch.Generator().manual_seed(11))
    info = dict(record_grads=True)
    D.optimize_instances(model, dev, inst, hp, sc0, tc0, seeds, opt_pose=True, sampling="grid", jitter=jit, info=info)
    got = [t.cpu().double() for t in info["code_grads"][0]]
    seen = []
    step = amd.ops.DeviceAdamW.step

    def recording_step(self):
        seen.append([p.grad.detach().cpu().double().clone() for p in self.params])
        return step(self)
    monkeypatch.setattr(amd.ops.DeviceAdamW, "step", recording_step)
    D.optimize_objects_batched(model, dev, views, hp, sc0.repeat(3, 1), tc0.repeat(3, 1), seeds, reg_iters=-1, jitter=jit)
    monkeypatch.undo()
    assert len(seen) == 1
    kw = dict(dtype=torch.float64, steps=False, to_matrix=D.axis_angle_to_matrix, to_vec=D.matrix_to_axis_angle)
    params = O.init_decoder_params()
    want = MR.fit(params, views, hp, sc0, tc0, seeds, jit, **kw)["grads"][0]
    rel = lambda a, b: float((a - b).abs().max()) / float(b.abs().max())
    single = 0.0
    for v in range(3):
        w1 = MR.fit(params, [views[v]], hp, sc0, tc0, [seeds[v]], jit[:, :, v:v + 1], **kw)["grads"][0]
        single = max(single, rel(seen[0][0][v:v + 1], w1[0]), rel(seen[0][1][v:v + 1], w1[1]))
    multi = max(rel(got[0], want[0]), rel(got[1], want[1]))
    print(f"shared-code gradient vs float64: {multi:.3e}; worst single-view gradient (batched loop): {single:.3e}; bound 3 x = {3 * single:.3e}")
    assert multi <= 3 * single


def test_padding_rays_are_neutral(amd, dev, model):
    """The 6 x 7-roi view with n_rays = 48 (6 padding rays) and with n_rays = 42 (none): iteration-0 loss, PSNR and code gradient agree to 1e-6
    relative (not bit for bit: the reduction over a view's rays is tiled by rays per object)."""
    D = amd.driver
    hp = hpams(D, num_opts=1)
    inst = D.make_instances([5], 1)
    inst[0]["views"][0] = small_view(amd, inst[0]["views"][0], 6, 7, 78)
    sc0, tc0 = start_codes(1, 5)
    p42 = D.draw_view_picks(inst[0]["views"], [3], 1, 42)
    p48 = torch.cat([p42, torch.full((1, 1, 6), -1, dtype=torch.int32)], dim=2)
    jit = torch.rand(1, 2, 1, 16, generator=torch.Generator().manual_seed(12))
    res = []
    for n, p in ((48, p48), (42, p42)):
        info = dict(record_grads=True)
        m, *_ = D.optimize_instances(model, dev, inst, hp, sc0, tc0, [51], n_rays=n, picks=p, jitter=jit, info=info)
        res.append((info["loss"][0, 0].cpu().double(), m[0, 0, 0].cpu().double(), info["code_grads"][0][0].cpu().double(), info["code_grads"][0][1].cpu().double()))
    for name, a, b in zip(("loss", "psnr", "d shape", "d texture"), *res):
        err = float((a - b).abs().max()) / float(b.abs().max())
        print(f"padding, {name}: relative difference {err:.2e}")
        assert err <= 1e-6, (name, err)


def test_fixed_poses(amd, dev, model):
    """opt_pose=False (optimize_objs_multi_anns): the poses come back unchanged, the rates are NOT halved (lr_half_interval = 2 would halve
    them twice in a loop that did), the traces follow the restatement."""
    D = amd.driver
    hp = hpams(D)
    hp["optimize"]["lr_half_interval"] = 2
    inst = D.make_instances([7], 2)
    views = inst[0]["views"]
    sc0, tc0 = start_codes(1, 6)
    jit = torch.rand(6, 2, 2, 16, generator=torch.Generator().manual_seed(13))
    m, sc, tc, pose = D.optimize_instances(model, dev, inst, hp, sc0, tc0, [61, 62], opt_pose=False, jitter=jit)
    assert torch.equal(pose.cpu(), torch.stack([v["cam_pose"] for v in views]))
    ref = MR.fit(O.init_decoder_params(), views, hp, sc0, tc0, [61, 62], jit, opt_pose=False)
    check_traces(m, ref)
    assert float(m[:, :, 2:].abs().max()) < 2e-3                                     # the true poses: no pose error
    d_codes = max(float((sc.cpu() - ref["codes"][-1][0]).abs().max()), float((tc.cpu() - ref["codes"][-1][1]).abs().max()))
    print("final codes |gpu - restatement|:", d_codes)
    assert d_codes < 2e-2                                                            # (four steps at half the rate would be 0.04 away)


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_multiview_loop_is_bit_reproducible(amd, dev, prec):
    """I = 2 with V = (3, 2), random sampling, twice: every output the same bits (the ordered segment sum has no atomics)."""
    D = amd.driver
    hp = hpams(D)
    assert amd.ops.split_supported(3, 1, 48 * 16)                                  # 48 rays x 16 samples per view: whole 32-point tiles
    m_ = amd.CodeNeRF(3, 1); m_.load_state_dict(O.init_decoder_params()); m_.precision = prec
    m_ = m_.to(dev)
    a, b = D.make_instances([2], 3)[0], D.make_instances([6], 2)[0]
    b["views"][1] = small_view(amd, b["views"][1], 6, 7, 79)
    sc0, tc0 = start_codes(2, 7)
    hp["n_rays"] = 48                                                              # (the reference's key; picks and jitter: the seeded defaults)
    runs = []
    for _ in range(2):
        out = D.optimize_instances(m_, dev, [a, b], hp, sc0, tc0, [71, 72, 73, 74, 75])
        torch.cuda.synchronize()
        runs.append([t.cpu() for t in out])
    for x, y in zip(*runs):
        assert torch.equal(x, y), float((x - y).abs().max())
    assert bool(torch.isfinite(runs[0][0]).all())


def test_ragged_batch_equals_its_instances_alone(amd, dev, model):
    """I = 2 with V = (1, 3) and different roi sizes: every instance as in a run of its own, within the batched-vs-single bands of
    test_batched_loop_equals_per_object_loop (1e-4 before the first step's drift; 0.05 dB and 2e-3 after)."""
    D = amd.driver
    hp = hpams(D)
    inst = [D.make_instances([4], 1)[0], D.make_instances([9], 3)[0]]
    sc0, tc0 = start_codes(2, 8)
    seeds = [81, 82, 83, 84]
    picks = D.draw_view_picks([v for i in inst for v in i["views"]], seeds, 6, 48)
    jit = torch.rand(6, 2, 4, 16, generator=torch.Generator().manual_seed(14))
    mb, scb, tcb, poseb = D.optimize_instances(model, dev, inst, hp, sc0, tc0, seeds, n_rays=48, picks=picks, jitter=jit)
    for i, (v0, v1) in enumerate(((0, 1), (1, 4))):
        m1, sc1, tc1, pose1 = D.optimize_instances(model, dev, inst[i:i + 1], hp, sc0[i:i + 1], tc0[i:i + 1], seeds[v0:v1], n_rays=48,
                                                   picks=picks[:, v0:v1], jitter=jit[:, :, v0:v1])
        d = (mb[v0:v1].cpu() - m1.cpu()).abs()
        assert float(d[:, :1].max()) < 1e-4, d[:, 0]
        assert float(d[:, :, 0].max()) < 0.05 and float(d[:, :, 2:].max()) < 2e-3, d
        assert float((poseb[v0:v1].cpu() - pose1.cpu()).abs().max()) < 2e-3 and float((scb[i].cpu() - sc1[0].cpu()).abs().max()) < 2e-2
