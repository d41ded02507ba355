"""The decoder kernels at the edges of their input range, against the float64 oracle.

Every other decoder test feeds coordinates in [-1, 1], weights at init scale, activations of order 1 and finite values.  Here:

A. coordinates up to 64 (and up to 1e4 for the exact kernels): the encodings' angles cross 1024, the seam of ``pe_sincos`` at 8192 (16.0
   at frequency 9, 32.0 at frequency 8) and reach the library branch, in every kernel that calls it, forward and backward;
B. decoders whose activations or weights are 2^-4 .. 2^-16 of init scale (tests/split_restatement.py): the split forward keeps fp16
   subnormal pieces (its error follows the CPU model that keeps them, far from the one that flushes them), and ``auto`` lets the
   scales through whose error stays inside ops.RANGE_TOL and downgrades the one that does not;
C. a NaN or an infinity in one point, direction or latent row: it changes no other point's output (bit for bit), and what the poisoned
   point itself returns is pinned -- the ReLU's v_med3 erases the NaN, so the point decodes as if that layer's output were 0.

Bands and mask matching: tests/oracle_bands.py, tests/relu_bits.py."""
import warnings

import pytest
import torch
import torch.nn.functional as F

import split_restatement as R
from oracle import supnerf_oracle as O
from oracle_bands import C_FP32, amd, check_all, check_per_ray, dev  # noqa: F401  (amd, dev: fixtures)
from relu_bits import decode_relu_bits
from test_precision_guard import _count_launches, _points

pytestmark = pytest.mark.gpu

SB, TB = 3, 1
MAGNITUDES = [0.7, 2.0, 15.999999, 16.0, 16.000002, 17.0, 31.999998, 32.0, 40.0, 64.0]


@pytest.fixture(scope="module")
def packed(amd, dev, oracle_params):
    return amd.ops.pack_weights({k: v.to(dev) for k, v in oracle_params.items()}, SB, TB)


# ================================================================== A. large coordinates
def _unit_dirs(P, g):
    return F.normalize(torch.randn(P, 3, generator=g), dim=-1)


def _large_points(P, draw, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    if draw == "seams":
        mag = torch.tensor(MAGNITUDES, dtype=torch.float32)[torch.randint(0, len(MAGNITUDES), (P, 3), generator=g)]
    else:                                                               # "far": 1e3 .. 1e4, log-uniform
        mag = (10.0 ** (3 + torch.rand(P, 3, generator=g))).float()
    sign = torch.randint(0, 2, (P, 3), generator=g).float() * 2 - 1
    return mag * sign, _unit_dirs(P, g), g


def _latent(params, B, g):
    sc, tc = torch.randn(B, 256, generator=g) * 0.3, torch.randn(B, 256, generator=g) * 0.3
    return O.latent_terms(params, sc, tc)


def _oracle_points(params, xyz, vd, lat, d_sig, d_rgb, bits, dt):
    """sigma, rgb and the gradients wrt xyz, viewdir and the latent terms on the oracle in ``dt``, with the ReLU bits of a launch."""
    p = {k: v.to(dt) for k, v in params.items()}
    x, v, z = [t.to(dt).clone().requires_grad_() for t in (xyz, vd, lat)]
    sig, rgb = O.decoder_forward(p, x[:, None], v[:, None], None, None, relu_masks=bits, latent=z)
    ((sig.reshape(-1) * d_sig.to(dt)).sum() + (rgb.reshape(-1, 3) * d_rgb.to(dt)).sum()).backward()
    return sig.detach().reshape(-1), rgb.detach().reshape(-1, 3), x.grad, v.grad, z.grad


def test_the_draw_reaches_the_seam_and_both_branches():
    xyz, _, _ = _large_points(384, "seams")
    ang = (xyz.abs()[:, None, :] * 2.0 ** torch.arange(10)[None, :, None]).reshape(-1, 30)      # [point][q = 3 frequency + axis]
    assert bool((ang == 8192.0).any()) and bool((ang == 1024.0).any())
    assert bool(((ang > 1024) & (ang < 8192)).any()) and bool((ang > 8192).any()) and bool((ang < 1).any())
    for first in (0, 1):                                                # pe_sincos2 takes (q, q + 1): pairs that straddle the seam, either parity
        a, b = ang[:, first:29:2], ang[:, first + 1:30:2]
        assert bool(((a <= 8192) != (b <= 8192)).any())


@pytest.mark.parametrize("draw", ["seams", "far"])
def test_encodings_at_large_coordinates(amd, dev, draw):
    """snr_pe_points and snr_encode_fwd's encodings (pe_points_kernel, encode_kernel, encode_dir_kernel)."""
    ops = amd.ops
    P = 384
    xyz, vd, _ = _large_points(P, draw)
    want = [torch.cat([O.positional_encoding(xyz.to(dt), 10), torch.zeros(P, 1, dtype=dt), O.positional_encoding(vd.to(dt), 4),
                       torch.zeros(P, 5, dtype=dt)], dim=1) for dt in (torch.float32, torch.float64)]
    out = ops.pe_points(xyz.to(dev), vd.to(dev))
    pairs = [("pe_points", out, want[0], want[1])]
    # the same points as samples of rays: sample 0 of ray r is point r exactly (origin = point * div, depth 0), sample 1 lies 8 further
    # along the ray; xyz_div = 1/32 brings origins of order 1 to these magnitudes
    div = 2.0 ** -5
    t = torch.tensor([0.0, 0.25])
    cfg = ops.RenderCfg(2, ops.Z_SHARED, P, SB, TB)
    e_xyz, e_vd, _, pe, ped = ops.encode((xyz * div).to(dev), vd.to(dev), t.to(dev), torch.tensor([div], device=dev), None, cfg, want_pe=True)
    assert torch.equal(e_xyz[:, 0].cpu(), xyz) and torch.equal(e_vd[:, 0].cpu(), vd)
    assert torch.equal(e_xyz.cpu(), (xyz[:, None] * div + vd[:, None] * t[None, :, None]) / div)
    pairs.append(("encode pe_xyz", pe, O.positional_encoding(e_xyz.cpu(), 10), O.positional_encoding(e_xyz.cpu().double(), 10)))
    pairs.append(("encode pe_dir", ped, O.positional_encoding(vd, 4), O.positional_encoding(vd.double(), 4)))
    check_all(pairs, "fp32")
    # sin / cos themselves, feature by feature (the bands above are relative to the largest raw coordinate)
    _check_features(f"pe_points {draw}", out[:, 3:63], xyz)
    _check_features(f"encode {draw}", pe[:, :, 3:63].reshape(-1, 60), e_xyz.reshape(-1, 3).cpu())


def _check_features(tag, feat, xyz):
    """Every sin / cos feature (P, 60) of the points ``xyz`` against float64: the fast branch within the 1.0e-7 its restatement keeps on
    the CPU (tests/test_split_restatement_cpu.py), the library branch within OpenCL's 4 ulp for sin / cos."""
    P = xyz.shape[0]
    angle = torch.cat([xyz.abs()[:, None, :] * 2.0 ** torch.arange(10)[None, :, None]] * 2, dim=1).reshape(P, 60)
    err = (feat.cpu().double() - O.positional_encoding(xyz.double(), 10)[:, 3:]).abs()
    fast = angle <= 8192
    print(f"[{tag}] max abs error against float64: fast branch {float(err[fast].max()):.2e}, library branch {float(err[~fast].max()):.2e}")
    assert bool(fast.any()) and bool((~fast).any())
    assert float(err[fast].max()) <= 1.0e-7 and float(err[~fast].max()) <= 4 * 2.0 ** -24


POINT_CASES = [("seams", 3, "fp32"), ("seams", 3, "bf16x3"), ("seams", 4, "fp32"), ("seams", 4, "bf16x3"), ("far", 3, "fp32"), ("far", 4, "fp32")]


@pytest.mark.parametrize("draw,B,precision", POINT_CASES)
def test_points_decoder_at_large_coordinates(amd, dev, oracle_params, packed, draw, B, precision):
    """decoder_fwd (plain and training kernels), density_fwd, decoder_bwd (both exact-fp32 kernels: 128 points per object without dumps
    take the 16x16 one, dumps or 96 points per object the 32x32 one) and density_bwd, mask-matched."""
    ops = amd.ops
    P = 384
    xyz, vd, g = _large_points(P, draw, seed=B)
    lat = _latent(oracle_params, B, g)
    d_sig, d_rgb = torch.randn(P, generator=g), torch.randn(P, 3, generator=g)
    x_d, v_d, l_d, ds_d, dr_d = [t.to(dev) for t in (xyz, vd, lat, d_sig, d_rgb)]
    sig, rgb, masks = ops.decoder_fwd(x_d, v_d, l_d, packed, SB, TB, save_masks=True, precision=precision)
    X = torch.full((SB + TB + 4, P, 256), float("nan"), device=dev)
    sig_t, rgb_t, masks_t = ops.decoder_fwd(x_d, v_d, l_d, packed, SB, TB, save_masks=True, precision=precision, activations=X)
    bits = decode_relu_bits(masks, P, SB, TB)
    o32, o64 = [_oracle_points(oracle_params, xyz, vd, lat, d_sig, d_rgb, bits, dt) for dt in (torch.float32, torch.float64)]
    x0 = [O.decoder_taps(oracle_params, xyz, vd, lat, d_sig, d_rgb, relu_masks=bits, dtype=dt)[0][0] for dt in (torch.float32, torch.float64)]
    pairs = [("sigma", sig, o32[0], o64[0]), ("rgb", rgb, o32[1], o64[1]), ("sigma (training kernel)", sig_t, o32[0], o64[0]),
             ("rgb (training kernel)", rgb_t, o32[1], o64[1]), ("X[0] (training kernel)", X[0], x0[0], x0[1])]
    if precision == "fp32":
        sig_d, masks_d = ops.density_fwd(x_d, l_d, packed, SB, TB, save_masks=True)
        assert torch.equal(sig_d, sig) and torch.equal(ops.density_fwd(x_d, l_d, packed, SB, TB)[0], sig)
    bad = []
    dumps = torch.empty(SB + TB + 4, P, 256, device=dev)
    for name, kw in (("", {}), (" (with layer dumps)", {"layer_grads": dumps})):
        d_lat, d_xyz, d_dir = ops.decoder_bwd(x_d, v_d, l_d, packed, masks, sig, ds_d, dr_d, SB, TB, precision=precision, **kw)
        pairs += [("d_viewdir" + name, d_dir, o32[3], o64[3]), ("d_latent" + name, d_lat, o32[4], o64[4])]
        bad += check_per_ray("d_xyz" + name, d_xyz, o32[2], o64[2])
    check_all(pairs, precision)
    assert not bad, bad
    if precision == "fp32":
        ref_lat, ref_xyz, _ = ops.decoder_bwd(x_d, v_d, l_d, packed, masks, sig, ds_d, torch.zeros_like(dr_d), SB, TB, need_dir=False,
                                              need_latent=(P // B) % 64 == 0, precision="fp32")
        dl, dx = ops.density_bwd(x_d, l_d, packed, masks_d, sig_d, ds_d, SB, TB, need_latent=(P // B) % 64 == 0)
        assert torch.equal(dx, ref_xyz) and bool(torch.isfinite(dx).all())
        if dl is not None:
            assert torch.equal(dl[:, :SB], ref_lat[:, :SB])
    torch.cuda.synchronize()


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_fused_render_at_large_coordinates(amd, dev, oracle_params, packed, precision):
    """Family A, 32 rays x 32 shared depths, xyz_div = 1/32: the samples run from the origins (up to 32 from the centre) 64 along the rays."""
    ops = amd.ops
    N = S = 32
    g = torch.Generator().manual_seed(7)
    div = 2.0 ** -5
    o = torch.rand(N, 3, generator=g) * 2 - 1
    d = _unit_dirs(N, g)
    t = torch.linspace(0.0, 2.0, S + 1)[:-1] + torch.rand(S, generator=g) * (2.0 / S)
    lat = _latent(oracle_params, 1, g)
    cfg = ops.RenderCfg(S, ops.Z_SHARED, N, SB, TB, precision=precision)
    out = ops.render_fwd(o.to(dev), d.to(dev), t.to(dev), torch.tensor([div], device=dev), None, lat.to(dev), packed, cfg)[:3]
    refs = []
    for dt in (torch.float32, torch.float64):
        xyz = (o.to(dt)[:, None] + d.to(dt)[:, None] * t.to(dt)[None, :, None]) / div
        if dt == torch.float32:
            ang = xyz.abs() * 512
            assert bool((ang > 8192).any()) and bool(((ang > 1024) & (ang <= 8192)).any()) and float(xyz.abs().max()) > 40
        sig, rgb = O.decoder_forward({k: v.to(dt) for k, v in oracle_params.items()}, xyz, d.to(dt)[:, None].expand(N, S, 3), None, None,
                                     latent=lat.to(dt))
        refs.append(O.composite(sig, rgb, t.to(dt)))
    check_all([(nm, a, b, c) for nm, a, b, c in zip(("rgb", "depth", "acc"), out, refs[0], refs[1])], precision)


# ================================================================== B. the split forward's low side
SCALES = [("activations", 4), ("activations", 8), ("activations", 16), ("weights", 4), ("weights", 8), ("weights", 16)]


def _guard_points():
    """test_precision_guard's 4096 points (64 x 64), directions and one code pair, on the CPU."""
    return _points(torch.device("cpu"))


@pytest.mark.parametrize("how,k", SCALES)
def test_split_forward_keeps_subnormal_pieces(amd, dev, oracle_params, how, k):
    """Kernel error against the float64 chain <= 4 x the error of the CPU model that KEEPS fp16 subnormal pieces (another sample of the same
    rounding noise: oracle_bands.C_FP32) + the exact kernels' own error on that decoder.  The model that flushes them is printed beside
    it: tests/test_split_restatement_cpu.py holds it 30 x above the kept one at k = 4."""
    ops = amd.ops
    assert ops.RANGE_TOL == 1e-5                                       # (the tolerance the CPU side derived the scales for)
    xyz, vd, sc, tc = _guard_points()
    xyz, vd = xyz.reshape(-1, 3), vd.reshape(-1, 3)
    params = R.scaled_decoder(oracle_params, how, k)
    lat = O.latent_terms(params, sc, tc)
    pk = ops.pack_weights({n: v.to(dev) for n, v in params.items()}, SB, TB)
    got = {p: ops.decoder_fwd(xyz.to(dev), vd.to(dev), lat.to(dev), pk, SB, TB, precision=p)[:2] for p in ("bf16x3", "fp32")}
    torch.cuda.synchronize()
    want = R.decoder_chain({n: v.double() for n, v in params.items()}, xyz, vd, lat.double(), R.lin_exact(torch.float64))
    e_split, e_fp32 = R.chain_error(got["bf16x3"], want), R.chain_error(got["fp32"], want)
    e_kept = R.chain_error(R.decoder_chain(params, xyz, vd, lat, R.lin_split_fp16()), want)
    e_flushed = R.chain_error(R.decoder_chain(params, xyz, vd, lat, R.lin_split_fp16(flush_subnormals=True)), want)
    print(f"[split low side] {how} 2^-{k}: split kernel {e_split:.2e}  fp32 kernel {e_fp32:.2e}  model keeping subnormals {e_kept:.2e}  "
          f"model flushing them {e_flushed:.2e}")
    assert all(bool(torch.isfinite(t).all()) for t in got["bf16x3"])   # at 2^-16 too: inaccurate, not broken
    assert e_split <= C_FP32 * e_kept + e_fp32, (e_split, e_kept, e_fp32, e_flushed)


def _module(amd, dev, params, precision=None):
    m = amd.CodeNeRF(SB, TB)
    m.load_state_dict(params)
    if precision is not None:
        m.precision = precision
    return m.to(dev)


@pytest.mark.parametrize("how,k", SCALES)
def test_auto_on_small_activations_and_weights(amd, dev, oracle_params, how, k):
    """``auto`` on a fresh module per scale: 2^-4 and 2^-8 pass the range guard silently; 2^-16 is downgraded to exact fp32 with one warning and
    returns the fp32 module's values bit for bit; one probe pair on the first call, none after; the fused render takes the same decision."""
    A = amd
    params = R.scaled_decoder(oracle_params, how, k)
    m = _module(A, dev, params)
    xyz, vd, sc, tc = [t.to(dev) for t in _guard_points()]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        with torch.no_grad():
            holder = {}
            n_first = _count_launches(lambda: holder.update(out=m(xyz, vd, sc, tc)))
            n_steady = _count_launches(lambda: m(xyz, vd, sc, tc))
    said = [w for w in caught if issubclass(w.category, RuntimeWarning)]
    assert n_first == 3 and n_steady == 1, (n_first, n_steady)
    rec, detail = m.last_precision, m._guard["detail"]
    print(f"[auto low side] {how} 2^-{k}: {rec['forward']}, {detail}")
    assert rec["requested"] == "auto"
    if k < 16:
        assert not said, [str(w.message) for w in said]
        assert rec["forward"] == "bf16x3" and "range guard passed" in rec["reason"]
        assert detail["values_out_of_tolerance"] == 0 and detail["weights_beyond_fp16_range"] == 0
    else:
        assert len(said) == 1 and "exact fp32 kernels" in str(said[0].message), [str(w.message) for w in said]
        assert rec["forward"] == "fp32" and rec["backward"] == "fp32" and "range guard" in rec["reason"]
        assert detail["values_out_of_tolerance"] > 0
        with torch.no_grad():
            want = _module(A, dev, params, "fp32")(xyz, vd, sc, tc)
        assert torch.equal(holder["out"][0], want[0]) and torch.equal(holder["out"][1], want[1])
    # the fused render: same module, same weight version -- no new probe, the same arithmetic
    ob = O.synthetic_object(11)
    img, mask = O.synthetic_targets(11, 16)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with torch.no_grad():
            n = _count_launches(lambda: A.utils.render_rays_v2(m, dev, img, mask, ob["cam_pose"].to(dev), ob["obj_diag"], ob["K"], ob["roi"], 64,
                                                               sc, tc, 1, 0, im_sz=16))
    assert n == 1 and m.last_precision["forward"] == ("bf16x3" if k < 16 else "fp32")


# ================================================================== C. non-finite inputs
POSITIONS = [0, 31, 32, 127, 128, 255]            # first and last lane of a tile, of a workgroup and of an object
POISONS = ["nan_xyz", "inf_xyz", "nan_dir"]
ERASED = ("the ReLU is v_med3(v, 0, +inf) (fmaxf in the fused exact-fp32 forward): with a NaN operand v_med3 returns min3, so a NaN "
          "pre-activation becomes 0 at the first ReLU behind the poison and the point decodes to finite values; torch.relu propagates the NaN")
PC, BC = 256, 2


def _poison_inputs():
    g = torch.Generator().manual_seed(41)
    xyz = torch.rand(PC, 3, generator=g) - 0.5
    vd = _unit_dirs(PC, g)
    d_sig, d_rgb = torch.randn(PC, generator=g), torch.randn(PC, 3, generator=g)
    return xyz, vd, g, d_sig, d_rgb


def _poisoned(kind, pos, xyz, vd):
    xyz, vd = xyz.clone(), vd.clone()
    if kind == "nan_xyz":
        xyz[pos, pos % 3] = float("nan")
    elif kind == "inf_xyz":
        xyz[pos, pos % 3] = float("inf")
    else:
        vd[pos, pos % 3] = float("nan")
    return xyz, vd


def _launch_all(ops, dev, packed, xyz, vd, lat, d_sig, d_rgb, precision):
    """Every decoder-points launch on these inputs: forward (plain and training), backward (plain and with layer dumps)."""
    x_d, v_d, l_d, ds_d, dr_d = [t.to(dev) for t in (xyz, vd, lat, d_sig, d_rgb)]
    n_slots = SB + TB + 4
    out = {}
    out["sigma"], out["rgb"], masks = ops.decoder_fwd(x_d, v_d, l_d, packed, SB, TB, save_masks=True, precision=precision)
    X = torch.zeros(n_slots, PC, 256, device=dev)
    out["sigma_train"], out["rgb_train"], masks_t = ops.decoder_fwd(x_d, v_d, l_d, packed, SB, TB, save_masks=True, precision=precision, activations=X)
    out["masks"], out["masks_train"], out["X"] = masks, masks_t, X
    out["d_latent"], out["d_xyz"], out["d_dir"] = ops.decoder_bwd(x_d, v_d, l_d, packed, masks, out["sigma"], ds_d, dr_d, SB, TB, precision=precision)
    G = torch.zeros(n_slots, PC, 256, device=dev)
    out["d_latent_dump"], out["d_xyz_dump"], out["d_dir_dump"] = ops.decoder_bwd(x_d, v_d, l_d, packed, masks, out["sigma"], ds_d, dr_d, SB, TB,
                                                                                 precision=precision, layer_grads=G)
    out["G"] = G
    torch.cuda.synchronize()                                            # (no launch returned an error code: ops.check raises; none faulted)
    return out


_CLEAN = {}


def _clean(ops, dev, packed, params, precision):
    if precision not in _CLEAN:
        xyz, vd, g, d_sig, d_rgb = _poison_inputs()
        lat = _latent(params, BC, g)
        _CLEAN[precision] = (xyz, vd, lat, d_sig, d_rgb, _launch_all(ops, dev, packed, xyz, vd, lat, d_sig, d_rgb, precision))
    return _CLEAN[precision]


def _assert_isolated(clean, dirty, keep_points, keep_objects, tag):
    """Bit equality of everything that belongs to the points ``keep_points`` (boolean (P,)) and the objects ``keep_objects``."""
    n_relu = SB + TB + 3
    for name in ("sigma", "rgb", "sigma_train", "rgb_train", "d_xyz", "d_dir", "d_xyz_dump", "d_dir_dump"):
        assert torch.equal(clean[name][keep_points], dirty[name][keep_points]), (tag, name)
    for name in ("X", "G"):
        for s in range(SB + TB + 4):
            w = 128 if s == SB + TB + 3 else 256
            assert torch.equal(clean[name][s][keep_points, :w], dirty[name][s][keep_points, :w]), (tag, name, s)
    for name in ("d_latent", "d_latent_dump"):
        assert torch.equal(clean[name][keep_objects], dirty[name][keep_objects]), (tag, name)
    keep_tiles = keep_points.reshape(-1, 32).all(1).to(clean["masks"].device)
    for name in ("masks", "masks_train"):
        a, b = [t[: PC // 32 * n_relu * 1024].reshape(PC // 32, -1) for t in (clean[name], dirty[name])]
        assert torch.equal(a[keep_tiles], b[keep_tiles]), (tag, name, "whole tiles")
        for la, lb in zip(decode_relu_bits(clean[name], PC, SB, TB), decode_relu_bits(dirty[name], PC, SB, TB)):
            assert torch.equal(la[keep_points.cpu()], lb[keep_points.cpu()]), (tag, name, "rows")


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("pos", POSITIONS)
@pytest.mark.parametrize("kind", POISONS)
def test_a_poisoned_point_changes_no_other_point(amd, dev, oracle_params, packed, kind, pos, precision):
    xyz, vd, lat, d_sig, d_rgb, clean = _clean(amd.ops, dev, packed, oracle_params, precision)
    px, pv = _poisoned(kind, pos, xyz, vd)
    dirty = _launch_all(amd.ops, dev, packed, px, pv, lat, d_sig, d_rgb, precision)
    keep = torch.ones(PC, dtype=torch.bool, device=dev)
    keep[pos] = False
    other = torch.tensor([b != pos // (PC // BC) for b in range(BC)], device=dev)
    _assert_isolated(clean, dirty, keep, other, (kind, pos, precision))
    if kind == "nan_dir":                                               # the density does not read the direction
        assert torch.equal(clean["sigma"], dirty["sigma"])


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_a_poisoned_latent_row_stays_in_its_object(amd, dev, oracle_params, packed, precision):
    xyz, vd, lat, d_sig, d_rgb, clean = _clean(amd.ops, dev, packed, oracle_params, precision)
    bad = lat.clone()
    bad[1, 1, 7] = float("nan")
    dirty = _launch_all(amd.ops, dev, packed, xyz, vd, bad, d_sig, d_rgb, precision)
    keep = torch.arange(PC, device=dev) < PC // BC
    _assert_isolated(clean, dirty, keep, torch.tensor([True, False], device=dev), ("nan_latent", precision))
    # the poisoned object itself: latent row 1 feeds shape_layer_2, whose ReLU erases the NaN -- its output is 0 for every point of the object
    rows = ~keep.cpu()
    want = [R.decoder_chain({n: v.to(dt) for n, v in oracle_params.items()}, xyz, vd, lat.to(dt), R.lin_exact(dt), zeroed={"shape_layer_2.0": rows})
            for dt in (torch.float32, torch.float64)]
    check_all([("sigma of the poisoned object", dirty["sigma"][~keep], want[0][0][rows], want[1][0][rows]),
               ("rgb of the poisoned object", dirty["rgb"][~keep], want[0][1][rows], want[1][1][rows])], precision)


def test_the_reference_propagates_the_poison(oracle_params):
    """The statement the parity tests below hold the kernels to, on the CPU oracle: NaN sigma and rgb for a poisoned coordinate, a finite
    sigma and NaN rgb for a poisoned direction."""
    xyz, vd, g, _, _ = _poison_inputs()
    lat = _latent(oracle_params, BC, g)
    for kind in POISONS:
        px, pv = _poisoned(kind, 31, xyz, vd)
        sig, rgb = O.decoder_forward(oracle_params, px[:, None], pv[:, None], None, None, latent=lat)
        assert bool(torch.isnan(rgb[31]).all()) and bool(torch.isnan(sig[31]).all()) == (kind != "nan_dir")
        keep = torch.arange(PC) != 31
        assert bool(torch.isfinite(sig[keep]).all()) and bool(torch.isfinite(rgb[keep]).all())


def _poisoned_outputs(amd, dev, oracle_params, packed, kind, precision):
    xyz, vd, lat, _, _, _ = _clean(amd.ops, dev, packed, oracle_params, precision)
    sigs, rgbs = [], []
    for pos in POSITIONS:
        px, pv = _poisoned(kind, pos, xyz, vd)
        sig, rgb, _ = amd.ops.decoder_fwd(px.to(dev), pv.to(dev), lat.to(dev), packed, SB, TB, precision=precision)
        sigs.append(sig[pos].cpu())
        rgbs.append(rgb[pos].cpu())
    torch.cuda.synchronize()
    return torch.stack(sigs), torch.stack(rgbs)


@pytest.mark.parametrize("precision", [pytest.param("fp32", marks=pytest.mark.xfail(strict=True, reason=ERASED)),
                                       pytest.param("bf16x3", marks=pytest.mark.xfail(strict=True, reason=ERASED))])
@pytest.mark.parametrize("kind", POISONS)
def test_a_poisoned_point_is_non_finite_like_the_reference(amd, dev, oracle_params, packed, kind, precision):
    """Reference parity: a poisoned point returns NaN, as torch.relu gives it (test_the_reference_propagates_the_poison)."""
    sig, rgb = _poisoned_outputs(amd, dev, oracle_params, packed, kind, precision)
    print(f"[poisoned point {kind} {precision}] sigma {sig.tolist()} rgb {rgb[0].tolist()}")
    assert not bool(torch.isfinite(rgb).any())
    if kind != "nan_dir":
        assert not bool(torch.isfinite(sig).any())


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("kind", POISONS)
def test_a_poisoned_point_decodes_as_a_zeroed_layer(amd, dev, oracle_params, packed, kind, precision):
    """The measured rule (include/supnerf_hip.h, "Input range"): the first ReLU behind the poison turns every NaN pre-activation into 0, so
    the point's outputs are the decoder's with that layer's output forced to 0 -- encoding_xyz's for a coordinate, encoding_viewdir's for
    a direction (whose density is the clean one) -- within the band of the arithmetic."""
    xyz, vd, lat, _, _, clean = _clean(amd.ops, dev, packed, oracle_params, precision)
    sig, rgb = _poisoned_outputs(amd, dev, oracle_params, packed, kind, precision)
    layer = "encoding_viewdir.0" if kind == "nan_dir" else "encoding_xyz.0"
    rows = torch.zeros(PC, dtype=torch.bool)
    rows[POSITIONS] = True
    want = [R.decoder_chain({n: v.to(dt) for n, v in oracle_params.items()}, xyz, vd, lat.to(dt), R.lin_exact(dt), zeroed={layer: rows})
            for dt in (torch.float32, torch.float64)]
    check_all([("sigma of the poisoned points", sig, want[0][0][POSITIONS], want[1][0][POSITIONS]),
               ("rgb of the poisoned points", rgb, want[0][1][POSITIONS], want[1][1][POSITIONS])], precision)
    if kind == "nan_dir":
        assert torch.equal(sig, clean["sigma"][POSITIONS].cpu())


# ------------------------------------------------------------------ the fused render
def _render_inputs():
    g = torch.Generator().manual_seed(43)
    N = S = 32
    o = (torch.rand(N, 3, generator=g) - 0.5) * 0.2
    d = _unit_dirs(N, g)
    t = torch.linspace(0.0, 0.5, S + 1)[:-1] + torch.rand(S, generator=g) * (0.5 / S)
    return o, d, t, g


def _render(amd, dev, oracle_params, packed, precision, poison_ray=None):
    ops = amd.ops
    o, d, t, g = _render_inputs()
    lat = _latent(oracle_params, 1, g)
    if poison_ray is not None:
        o = o.clone()
        o[poison_ray, 1] = float("nan")
    cfg = ops.RenderCfg(32, ops.Z_SHARED, 32, SB, TB, precision=precision)
    out = ops.render_fwd(o.to(dev), d.to(dev), t.to(dev), torch.ones(1, device=dev), None, lat.to(dev), packed, cfg)[:3]
    torch.cuda.synchronize()
    return (o, d, t, lat), out


POISON_RAY = 13


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_a_poisoned_ray_changes_no_other_ray(amd, dev, oracle_params, packed, precision):
    _, clean = _render(amd, dev, oracle_params, packed, precision)
    _, dirty = _render(amd, dev, oracle_params, packed, precision, POISON_RAY)
    keep = torch.arange(32, device=dev) != POISON_RAY
    for name, a, b in zip(("rgb", "depth", "acc"), clean, dirty):
        assert torch.equal(a[keep], b[keep]), (name, precision)


@pytest.mark.parametrize("precision", [pytest.param("fp32", marks=pytest.mark.xfail(strict=True, reason=ERASED)),
                                       pytest.param("bf16x3", marks=pytest.mark.xfail(strict=True, reason=ERASED))])
def test_a_poisoned_ray_is_non_finite_like_the_reference(amd, dev, oracle_params, packed, precision):
    (o, d, t, lat), out = _render(amd, dev, oracle_params, packed, precision, POISON_RAY)
    xyz = o[:, None] + d[:, None] * t[None, :, None]
    sig, rgb = O.decoder_forward(oracle_params, xyz, d[:, None].expand(32, 32, 3), None, None, latent=lat)
    ref = O.composite(sig, rgb, t)
    assert all(bool(torch.isnan(r[POISON_RAY]).all()) for r in ref)          # the reference's answer
    print(f"[poisoned ray {precision}] rgb {out[0][POISON_RAY].tolist()} depth {float(out[1][POISON_RAY])} acc {float(out[2][POISON_RAY])}")
    assert not any(bool(torch.isfinite(x[POISON_RAY]).any()) for x in out)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_a_poisoned_ray_renders_a_zeroed_first_layer(amd, dev, oracle_params, packed, precision):
    """The rule of the points decoder inside the fused launch: every sample of the poisoned ray decodes with encoding_xyz's output 0."""
    (o, d, t, lat), out = _render(amd, dev, oracle_params, packed, precision, POISON_RAY)
    S = 32
    refs = []
    for dt in (torch.float32, torch.float64):
        zero_xyz = torch.zeros(S, 3)                                    # (any finite point: the layer's output is forced to 0)
        sig, rgb = R.decoder_chain({n: v.to(dt) for n, v in oracle_params.items()}, zero_xyz, d[POISON_RAY].expand(S, 3), lat.to(dt),
                                   R.lin_exact(dt), zeroed={"encoding_xyz.0": torch.ones(S, dtype=torch.bool)})
        refs.append(O.composite(sig[None], rgb[None], t.to(dt)))
    check_all([(nm, a[POISON_RAY:POISON_RAY + 1], b, c) for nm, a, b, c in zip(("rgb", "depth", "acc"), out, refs[0], refs[1])], precision)
