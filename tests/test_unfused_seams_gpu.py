"""The two ends of the unfused render chain -- ``snr_composite_fwd`` / ``snr_composite_bwd`` and ``snr_encode_fwd``'s positional encodings
(csrc/snr_aux.hip) -- at their seams, against the float64 oracle.  Inputs, references and the judgement are those of
tests/unfused_seam_cases.py; tests/test_unfused_seams_cpu.py shows that the judgement sees a kernel that is wrong at one seam.

a. ``composite_fwd16_kernel`` (16 lanes per ray, four rays per wave) with rows of lanes that S does not fill (S = 4 .. 60), groups of
   four rays that N does not fill, and per-object depths whose object boundary falls at every place inside a group; the backward on the
   same launches, with d_sigma exactly 0.0 on densities <= 0.
b. The alignment fallback: an operand 4 bytes off sends an S the 16-lane kernel owns to ``composite_fwd_kernel``.
c. A ray's results do not depend on its slot in the group or the wave: the same bits wherever it stands.
d. The second trip of the grid-stride loops of ``composite_fwd16_kernel``, ``composite_fwd_kernel`` and ``composite_bwd_kernel``, through
   the C ABI into NaN-filled buffers of the test's own with a canary tail.
e. S > 256: the forward carries across 64-sample chunks, the backward refuses.
f. ``encode_kernel``'s positional-encoding phase and ``encode_dir_kernel`` on ragged last blocks, at a 16-byte aligned output and one
   4 bytes further (the scalar store path), through the C ABI into NaN-filled buffers with a canary tail.

Room when written (MI355X), largest error over band: (a) 0.067 (S = 36; no S above that), (b) 0.017, (d) 0.013 (the backward at S = 8;
the two forwards 0.008), (e) 0.071; (f) 8.9e-8 on pe_xyz and 8.1e-8 on pe_dir, 0.18 of the 5e-7 bound.  No seam moved a bit: (b)'s four
misaligned variants, (c)'s rolled rays, (d)'s second trips and (f)'s two store paths agree exactly."""
import ctypes as C
import math

import pytest
import torch

import unfused_seam_cases as SC
from oracle import supnerf_oracle as O
from oracle_bands import amd, dev, md  # noqa: F401  (amd, dev: fixtures)

pytestmark = pytest.mark.gpu

CANARY = 1024                       # floats behind every caller-owned output: 4 KiB
SENTINEL = -7.0e7


def z_mode_of(ops, mode):
    return {"shared": ops.Z_SHARED, "per_object": ops.Z_PER_OBJECT, "per_ray": ops.Z_PER_RAY}[mode]


def run(ops, dev, sig, rgbs, zt, wts, mode, rpo, white, backward=True):
    """The public route: ``ops.Composite`` and autograd of sum_i (out_i * w_i), or ``ops.composite_fwd`` alone -> a dict over ``SC.NAMES``."""
    if not backward:
        return dict(zip(SC.OUTPUTS, ops.composite_fwd(sig.to(dev), rgbs.to(dev), zt.to(dev), z_mode_of(ops, mode), white, rpo)))
    lv = [sig.to(dev).requires_grad_(), rgbs.to(dev).requires_grad_(), zt.to(dev).requires_grad_(mode == "per_ray")]
    out = ops.Composite.apply(*lv, z_mode_of(ops, mode), white, rpo)
    sum((a.reshape(w.shape) * w.to(dev)).sum() for a, w in zip(out, wts)).backward()
    res = {k: v.detach() for k, v in zip(SC.OUTPUTS, out)}
    res.update(d_sigma=lv[0].grad, d_rgbs=lv[1].grad, d_z=lv[2].grad if mode == "per_ray" else None)
    return res


# ------------------------------------------------------------------ a. lane groups
@pytest.mark.parametrize("S", [4, 8, 12, 16, 20, 32, 36, 48, 60, 64])
def test_lane_group_sweep(amd, dev, S):
    ops = amd.ops
    worst = 0.0
    launches = [(N, mode, 0) for N in (1, 2, 3, 4, 5, 7, 8, 9) for mode in ("shared", "per_ray")]
    launches += [(B * rpo, "per_object", rpo) for rpo in (1, 3, 5) for B in (2, 3)]          # boundaries at every place inside a group of four
    for N, mode, rpo in launches:
        sig, rgbs, z, wts = SC.seam_inputs(N, S, 1000 * S + 10 * N + rpo)
        zt = SC.depth_table(z, mode, rpo)
        if mode == "per_object":
            assert zt.shape == (N // rpo, S) and not any(torch.equal(zt[a], zt[b]) for a in range(len(zt)) for b in range(a))
        for white in (True, False):
            got = run(ops, dev, sig, rgbs, zt, wts, mode, rpo, white)
            r32, r64 = SC.references(sig, rgbs, zt, wts, mode, rpo, white)
            worst = max(worst, SC.judge(f"S={S} N={N} {mode} rays_per_obj={rpo} white={white}", got, r32, r64, sig))
    print(f"[seams a] S={S}: largest error / band {worst:.3f}")


# ------------------------------------------------------------------ b. alignment fallback
def off_by_one_float(t, dev):
    """``t`` as a dense view that starts one float into a larger buffer: 4 bytes off a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, device=dev)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("S", [4, 32, 60])
def test_alignment_fallback(amd, dev, S):
    """csrc/snr_aux.hip ``snr_composite_fwd``: ``aligned`` is false as soon as one of sigmas, rgbs, z_vals is not 16-byte aligned, and the
    launch goes to ``composite_fwd_kernel`` -- the same kernel, so the same bits, whichever operand it was.  (``_f32c`` keeps a dense
    view as it is.)  The 16-lane kernel's bits are not demanded: its products associate differently."""
    ops = amd.ops
    N = 7
    worst = 0.0
    for mode in ("per_ray", "shared"):
        sig, rgbs, z, wts = SC.seam_inputs(N, S, 77 + S)
        zt = SC.depth_table(z, mode)
        r32, r64 = SC.references(sig, rgbs, zt, wts, mode, 0, True, backward=False)
        dense = [t.to(dev) for t in (sig, rgbs, zt)]
        assert all(t.data_ptr() % 16 == 0 for t in dense)
        results = []
        for off in ((0,), (1,), (2,), (0, 1, 2)):
            ins = [off_by_one_float(t, dev) if i in off else t for i, t in enumerate(dense)]
            assert all(ops._f32c(t).data_ptr() == t.data_ptr() for t in ins)
            got = dict(zip(SC.OUTPUTS, ops.composite_fwd(*ins, z_mode_of(ops, mode), True)))
            worst = max(worst, SC.judge(f"S={S} {mode} misaligned {off}", got, r32, r64, sig))
            results.append(got)
        for got in results[1:]:
            assert all(torch.equal(got[k], results[0][k]) for k in SC.OUTPUTS), mode
        aligned = dict(zip(SC.OUTPUTS, ops.composite_fwd(*dense, z_mode_of(ops, mode), True)))
        worst = max(worst, SC.judge(f"S={S} {mode} aligned", aligned, r32, r64, sig))
    print(f"[seams b] S={S}: largest error / band {worst:.3f}")


# ------------------------------------------------------------------ c. position independence
@pytest.mark.parametrize("S", [12, 64, 65])
def test_position_independence(amd, dev, S):
    ops = amd.ops
    N = 11
    sig, rgbs, z, wts = SC.seam_inputs(N, S, 500 + S)
    base = run(ops, dev, sig, rgbs, z, wts, "per_ray", 0, True)
    r32, r64 = SC.references(sig, rgbs, z, wts, "per_ray", 0, True)
    SC.judge(f"S={S}", base, r32, r64, sig)
    for shift in (1, 2, 3):
        perm = torch.arange(N).roll(shift)
        moved = run(ops, dev, sig[perm], rgbs[perm], z[perm], [w[perm] for w in wts], "per_ray", 0, True)
        assert SC.position_mismatches(base, moved, perm) == [], shift


# ------------------------------------------------------------------ d. grid stride, caller-owned outputs
# csrc/snr_aux.hip, snr_composite_fwd:  grid_for(n_rays * 16, 256, 16384) workgroups of 256 threads, 16 lanes per ray
#                                       grid_for(n_rays * 64, 256, 8192) for composite_fwd_kernel, 64 lanes per ray
#                  snr_composite_bwd:   grid_for(n_rays * 64, 256, 8192), 64 lanes per ray
# so one trip of the grid-stride loop covers cap * 256 / lanes_per_ray rays:
SWEEP_16_LANES = 16384 * 256 // 16
SWEEP_64_LANES = 8192 * 256 // 64


def guarded(dev, guards, *shape):
    n = math.prod(shape)
    buf = torch.full((n + CANARY,), float("nan"), device=dev)
    buf[n:] = SENTINEL
    guards.append((buf, n))
    return buf[:n].view(shape)


def canaries_intact(guards):
    return all(bool((buf[n:] == SENTINEL).all()) for buf, n in guards)


def abi_composite(amd, dev, sig, rgbs, zt, wts, mode, white, forward, backward):
    """``snr_composite_fwd`` / ``snr_composite_bwd`` through the C ABI, every output NaN-filled with a canary tail -> a dict over the names
    of the halves that ran."""
    ops, lib = amd.ops, amd._lib.lib()
    N, S = sig.shape
    ins = [t.to(dev).contiguous() for t in (sig, rgbs, zt)]
    assert all(t.data_ptr() % 16 == 0 for t in ins)
    ups = [w.to(dev).contiguous() for w in wts]
    flags = ops.WHITE_BKGD if white else 0
    guards, res = [], {}
    if forward:
        outs = [guarded(dev, guards, N, 3), guarded(dev, guards, N), guarded(dev, guards, N)]
        assert lib.snr_composite_fwd(*[ops._p(t) for t in ins], z_mode_of(ops, mode), flags, N, 0, S, *[ops._p(t) for t in outs], ops._stream(dev)) == 0
        res.update(zip(SC.OUTPUTS, outs))
    if backward:
        gs = [guarded(dev, guards, N, S), guarded(dev, guards, N, S, 3), guarded(dev, guards, N, S) if mode == "per_ray" else None]
        assert lib.snr_composite_bwd(*[ops._p(t) for t in ins], z_mode_of(ops, mode), flags, N, 0, S, *[ops._p(t) for t in ups],
                                     *[ops._p(t) for t in gs], ops._stream(dev)) == 0
        res.update(zip(("d_sigma", "d_rgbs", "d_z"), gs))
    torch.cuda.synchronize()
    assert canaries_intact(guards), "a composite kernel stored behind one of its outputs"
    return res


@pytest.mark.parametrize("mode", ["per_ray", "shared"])
@pytest.mark.parametrize("S,N,sweep,forward,backward", [(4, 262144 + 5, SWEEP_16_LANES, True, False), (2, 32768 + 3, SWEEP_64_LANES, True, True),
                                                        (8, 32768 + 3, SWEEP_64_LANES, False, True)])
def test_grid_stride_second_trip(amd, dev, S, N, sweep, forward, backward, mode):
    # the premise: which kernel the dispatch picks for this S, and that N is one trip plus a little
    lanes = 16 if forward and S <= 64 and S % 4 == 0 else 64
    assert sweep == {16: 262144, 64: 32768}[lanes] and 0 < N - sweep < 8 and (lanes == 64 or N - sweep > 4)
    assert not backward or S <= 64
    sig, rgbs, z, wts = SC.seam_inputs(N, S, S)
    zt = SC.depth_table(z, mode)
    worst = 0.0
    for white in (True, False):
        got = abi_composite(amd, dev, sig, rgbs, zt, wts, mode, white, forward, backward)
        r32, r64 = [SC.reference(sig, rgbs, zt, wts, mode, 0, white, dt, backward) for dt in (torch.float32, torch.float64)]
        if not forward:
            r32, r64 = [{k: v for k, v in r.items() if k not in SC.OUTPUTS} for r in (r32, r64)]
        worst = max(worst, SC.judge(f"S={S} N={N} {mode} white={white}", got, r32, r64, sig))          # (finite: every element was written)
        head = abi_composite(amd, dev, sig[sweep:], rgbs[sweep:], zt[sweep:] if mode == "per_ray" else zt, [w[sweep:] for w in wts], mode, white,
                             forward, backward)
        assert SC.trip_mismatches(got, head, sweep) == []
    print(f"[seams d] S={S} N={N} {mode}: largest error / band {worst:.3f}")


# ------------------------------------------------------------------ e. long rays
@pytest.mark.parametrize("S", [257, 320])
def test_long_rays_forward(amd, dev, S):
    ops = amd.ops
    sig, rgbs, z, wts = SC.seam_inputs(5, S, S)
    worst = 0.0
    for white in (True, False):
        got = run(ops, dev, sig, rgbs, z, wts, "per_ray", 0, white, backward=False)
        r32, r64 = SC.references(sig, rgbs, z, wts, "per_ray", 0, white, backward=False)
        worst = max(worst, SC.judge(f"S={S} white={white}", got, r32, r64, sig))
    print(f"[seams e] S={S}: largest error / band {worst:.3f}")


def test_long_rays_backward_is_refused(amd, dev):
    """``snr_composite_bwd`` returns SNR_E_UNSUPPORTED for S > 256 before any launch."""
    ops = amd.ops
    sig, rgbs, z, wts = SC.seam_inputs(5, 257, 257)
    with pytest.raises(amd.SnrError):
        ops.composite_bwd(sig.to(dev), rgbs.to(dev), z.to(dev), ops.Z_PER_RAY, True, 0, *[w.to(dev) for w in wts], True)
    lv = [t.to(dev).requires_grad_() for t in (sig, rgbs, z)]
    out = ops.Composite.apply(*lv, ops.Z_PER_RAY, True, 0)
    with pytest.raises(amd.SnrError):
        out[0].sum().backward()


# ------------------------------------------------------------------ f. the encodings on ragged blocks
PE_TOL = 5e-7          # test_pe_points_layout's bound for the same pe_sincos (9.2e-8 of float64 per value, the CPU's sin / cos likewise)


def offset_output(dev, guards, n, floats_off):
    """A NaN-filled output of ``n`` floats that starts ``floats_off`` floats behind a 16-byte boundary, with a canary tail."""
    buf = torch.full((floats_off + n + CANARY,), float("nan"), device=dev)
    buf[floats_off + n:] = SENTINEL
    guards.append((buf, floats_off + n))
    v = buf[floats_off:floats_off + n]
    assert buf.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 4 * floats_off
    return v


@pytest.mark.parametrize("flags", [(False, False, False), (False, True, False)], ids=["identity", "kitti2nusc"])
@pytest.mark.parametrize("N,S", [(1, 1), (127, 1), (129, 1), (43, 3), (85, 3), (128, 3), (55, 7), (3, 48), (19, 1)])
def test_encode_pe_on_ragged_blocks(amd, dev, N, S, flags):
    """``encode_kernel``: blocks of 256 points in two passes of 128 through LDS, 16-byte stores with a scalar tail, scalar stores when
    pe_xyz is not 16-byte aligned; ``encode_dir_kernel``: one thread per element of (N, 27).  P = N S and 27 N on both sides of the block
    sizes.  Shared depths, xyz_div = 2, |xyz| <= 1: angles up to 512."""
    ops, lib = amd.ops, amd._lib.lib()
    frame = amd.utils._frame(*flags)
    g = torch.Generator().manual_seed(100 * N + S)
    rays_o = torch.rand(N, 3, generator=g) * 2 - 1
    rays_d = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    t = torch.sort(torch.rand(S, generator=g))[0]
    ins = [x.to(dev).contiguous() for x in (rays_o, rays_d, t, torch.tensor([2.0]))]
    a = ops._render_args(*ins, None, None, None, frame, 1.0, ops.Z_SHARED, 0, N, S, 0, 0)
    P = N * S
    results = []
    for floats_off in (0, 1):
        guards = []
        xyz, vd, z = guarded(dev, guards, P, 3), guarded(dev, guards, P, 3), guarded(dev, guards, P)
        pe, ped = offset_output(dev, guards, P * 63, floats_off), offset_output(dev, guards, N * 27, floats_off)
        assert lib.snr_encode_fwd(C.byref(a), *[ops._p(x) for x in (xyz, vd, z, pe, ped)], ops._p(None), ops._stream(dev)) == 0
        torch.cuda.synchronize()
        assert canaries_intact(guards), f"snr_encode_fwd stored behind one of its outputs (pe_xyz {4 * floats_off} bytes off)"
        results.append([x.cpu() for x in (xyz, vd, pe.view(P, 63), ped.view(N, 27))])
    (xyz, vd, pe, ped), again = results
    for x, y, name in zip(results[0], again, ("xyz", "viewdir", "pe_xyz", "pe_dir")):
        assert bool(torch.isfinite(x).all()), name
        assert torch.equal(x, y), f"{name}: the aligned and the misaligned call differ"
    assert float(xyz.abs().max()) <= 1.0
    assert torch.equal(pe[:, :3], xyz)
    e_xyz = md(pe, O.positional_encoding(xyz.double(), 10))
    M = torch.tensor(frame, dtype=torch.float64).reshape(3, 3)
    v = rays_d.double() @ M.T                              # a signed permutation: exact
    assert torch.equal(ped[:, :3].double(), v) and torch.equal(ped[:, :3], vd.view(N, S, 3)[:, 0])
    e_dir = md(ped, O.positional_encoding(v, 4))
    print(f"[seams f] N={N} S={S}: pe_xyz {e_xyz:.2e}, pe_dir {e_dir:.2e} of {PE_TOL:.0e}: largest error / bound {max(e_xyz, e_dir) / PE_TOL:.3f}")
    assert e_xyz < PE_TOL and e_dir < PE_TOL
