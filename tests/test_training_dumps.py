"""The training path's HBM dumps and the weight gradients built from them, at every block count, against the float64 oracle, mask-matched.

In training mode (``model.train_decoder_weights``, ``ops.DecoderPointsTrain``) the layer chains write every MFMA layer's input X_l (forward,
``activations``) and every layer's pre-activation gradient G_l (backward, ``layer_grads``); the weight gradients are G_l^T X_{l-1} from
``ops.weight_grad``.  Four kernel instantiations serve only this path (chosen by ``decoder_forward`` / ``decoder_backward``, csrc/snr_decoder.hip):
* fp32: ``decoder_train_fwd_kernel`` (csrc/snr_mlp.hip; latent rows staged in LDS up to LDS_LAT_ROWS = 8, read from memory beyond) and
  ``decoder_bwd_kernel<0>`` with ``io.gdump`` (csrc/snr_mlp_bwd.hip; ``snr_fp32_bwd16_supported_`` refuses dumps);
* split: ``bf16_fwd_kernel<0, true, false, true>`` and ``bf16_bwd16_kernel<0, true>`` (csrc/snr_bf16.hip), <= 4 blocks and whole 32-point
  tiles per object.
The oracle's ``decoder_taps`` gives the same slots (tests/test_oracle_taps.py checks that they rebuild autograd's weight gradients).

Bands of tests/oracle_bands.py: |got - f64| <= C |fp32 oracle - f64| + floor, relative to the tensor's largest float64 entry, with
C = 4 for the fp32 kernels and 32 for the split ones.  Dumps live at the front of NaN-filled buffers with a guard behind them: every live row
must be written and finite, and nothing may be written past the end."""
import pytest
import torch
import torch.nn.functional as F

from oracle import supnerf_oracle as O
from oracle_bands import amd, band_of, check_all, dev, make_model  # noqa: F401  (amd, dev: fixtures)
from relu_bits import decode_relu_bits, relu_bits_of

pytestmark = pytest.mark.gpu

GUARD = 16384            # floats (64 KiB) of NaN behind every dump


def arith(precision):
    """(forward, backward) arithmetic names of a direct launch pair."""
    return {"fp32": ("fp32", "fp32"), "bf16x3": ("bf16x3", "bf16x3"), "fp32-split": ("fp32", "bf16x3")}[precision]


def split_takes(sb, tb, per_obj):
    """csrc/snr_bf16.hip snr_bf16_supported_ (checked against the library in every test that relies on it)."""
    return sb + tb <= 4 and per_obj % 32 == 0


def make_inputs(sb, tb, B, n, seed):
    """Points, directions, distinct latent terms per object and distinct upstream weights per object."""
    g = torch.Generator().manual_seed(seed)
    P = B * n
    xyz = torch.rand(P, 3, generator=g) * 2 - 1
    vd = F.normalize(torch.randn(P, 3, generator=g), dim=-1)
    lat = torch.relu(torch.randn(B, max(sb + tb, 1), 256, generator=g) * 0.3 + 0.05 * torch.arange(B)[:, None, None])
    if sb + tb == 0:
        lat.zero_()                # (the model's dummy row)
    scale = (1.0 + torch.arange(B, dtype=torch.float32)).repeat_interleave(n)
    d_sig = torch.randn(P, generator=g) * scale
    d_rgb = torch.randn(P, 3, generator=g) * scale[:, None]
    return xyz, vd, lat, d_sig, d_rgb


def nan_dump(n_slots, P, dev):
    """(buffer, dump view at its front): (n_slots, P, 256) floats, then GUARD floats; all NaN."""
    buf = torch.full((n_slots * P * 256 + GUARD,), float("nan"), device=dev)
    return buf, buf[: n_slots * P * 256].view(n_slots, P, 256)


def slot_width(s, n_slots):
    return 128 if s == n_slots - 1 else 256


def check_written(buf, D, what):
    """Every live row of every slot finite (columns 128.. of the 128-wide slot unread); the guard behind the dump untouched."""
    n_slots, P = D.shape[:2]
    for s in range(n_slots):
        bad = int((~torch.isfinite(D[s, :, :slot_width(s, n_slots)])).any(1).sum())
        assert bad == 0, f"{what} slot {s}: {bad} of {P} rows not finite (never written?)"
    assert bool(torch.isnan(buf[n_slots * P * 256:]).all()), f"{what}: written past the end of the dump"


def launch(amd, dev, params, sb, tb, xyz, vd, lat, d_sig, d_rgb, precision, need_latent=True):
    """The training launch pair with NaN-guarded dumps; returns (X buffer, X, G buffer, G, ReLU bits decoded)."""
    ops = amd.ops
    fwd, bwd = arith(precision)
    packed = ops.pack_weights({k: v.to(dev) for k, v in params.items()}, sb, tb)
    P, n_slots = xyz.shape[0], sb + tb + 4
    xbuf, X = nan_dump(n_slots, P, dev)
    gbuf, G = nan_dump(n_slots, P, dev)
    x_d, v_d, l_d = xyz.to(dev), vd.to(dev), lat.to(dev)
    sig, _, masks = ops.decoder_fwd(x_d, v_d, l_d, packed, sb, tb, save_masks=True, precision=fwd, activations=X)
    ops.decoder_bwd(x_d, v_d, l_d, packed, masks, sig, d_sig.to(dev), d_rgb.to(dev), sb, tb, need_latent=need_latent, precision=bwd,
                    layer_grads=G)
    torch.cuda.synchronize()
    return xbuf, X, gbuf, G, masks


def taps(params, xyz, vd, lat, d_sig, d_rgb, masks):
    """The fp32 and float64 oracle slots, mask-matched: {dtype: (X, G)}."""
    out = {}
    for dt in (torch.float32, torch.float64):
        X, G, _ = O.decoder_taps(params, xyz, vd, lat, d_sig, d_rgb, relu_masks=masks, dtype=dt)
        out[dt] = (X, G)
    return out


def compare_dumps(X, G, ref, precision, rows=None, tag=""):
    fwd, bwd = arith(precision)
    n_slots = X.shape[0]
    pairs_x, pairs_g = [], []
    for s in range(n_slots):
        w = slot_width(s, n_slots)
        gx, gg = (X[s, :, :w], G[s, :, :w]) if rows is None else (X[s, rows, :w], G[s, rows, :w])
        pairs_x.append((f"{tag}X[{s}]", gx.cpu(), ref[torch.float32][0][s], ref[torch.float64][0][s]))
        pairs_g.append((f"{tag}G[{s}]", gg.cpu(), ref[torch.float32][1][s], ref[torch.float64][1][s]))
    check_all(pairs_x, band_of(fwd))
    check_all(pairs_g, band_of(bwd))


# ------------------------------------------------------------------ a. the dumps themselves
BOTH_BLOCKS = [(0, 0), (1, 0), (0, 1), (2, 1), (3, 1), (2, 2), (0, 4), (4, 0)]
FP32_BLOCKS = [(4, 4), (5, 4), (5, 5), (8, 8)]          # 8 latent rows: staged in LDS; 9 and more: read from memory
SHAPES = [(1, 32), (3, 96), (2, 4096)]                   # one partial workgroup; workgroups straddle objects (P % 128 = 32); many
DUMP_CASES = [(sb, tb, B, n, prec) for sb, tb in BOTH_BLOCKS for B, n in SHAPES for prec in ("fp32", "fp32-split", "bf16x3")]
DUMP_CASES += [(sb, tb, B, n, "fp32") for sb, tb in FP32_BLOCKS for B, n in SHAPES]
_ORACLE = {}             # the last oracle, keyed by the case and the ReLU bits it was matched to (fp32 and fp32-split share it)


def oracle_for(key, params, ins, bits):
    hit = _ORACLE.get("entry")
    if hit is not None and hit[0] == key and all(torch.equal(a, b) for a, b in zip(hit[1], bits)):
        return hit[2]
    _ORACLE.pop("entry", None)
    ref = taps(params, *ins, bits)
    _ORACLE["entry"] = (key, bits, ref)
    return ref


@pytest.mark.parametrize("sb,tb,B,n,precision", DUMP_CASES, ids=lambda v: str(v))
def test_dumps_match_the_oracle(amd, dev, sb, tb, B, n, precision):
    if precision != "fp32":
        assert amd.ops.split_supported(sb, tb, n) == split_takes(sb, tb, n)
    params = O.init_decoder_params(sb, tb, seed=40 + sb + 10 * tb)
    ins = make_inputs(sb, tb, B, n, seed=1000 * sb + 100 * tb + B)
    xbuf, X, gbuf, G, masks = launch(amd, dev, params, sb, tb, *ins, precision)
    check_written(xbuf, X, "X")
    check_written(gbuf, G, "G")
    bits = decode_relu_bits(masks, B * n, sb, tb)
    ref = oracle_for((sb, tb, B, n, arith(precision)[0]), params, ins, bits)
    compare_dumps(X, G, ref, precision)


@pytest.mark.parametrize("sb,tb", [(0, 0), (3, 1)])
@pytest.mark.parametrize("P", [1, 33, 70, 1000])
def test_dumps_ragged_point_counts(amd, dev, sb, tb, P):
    """One object of P points, no latent gradient: the fp32 kernels' last wave tile has P % 32 live rows (dump_rows < 32)."""
    params = O.init_decoder_params(sb, tb, seed=7)
    ins = make_inputs(sb, tb, 1, P, seed=P)
    xbuf, X, gbuf, G, masks = launch(amd, dev, params, sb, tb, *ins, "fp32", need_latent=False)
    check_written(xbuf, X, "X")
    check_written(gbuf, G, "G")
    compare_dumps(X, G, taps(params, *ins, decode_relu_bits(masks, P, sb, tb)), "fp32")


# ------------------------------------------------------------------ b. end to end through the model
E2E_BLOCKS = [(0, 0), (1, 0), (2, 1), (0, 4), (2, 2), (5, 5), (8, 8)]
BATCHES = {"whole": (3, 4, 16), "ragged": (2, 5, 7)}       # objects, rays per object, samples per ray
TRIPLE = ("fp32", "bf16x3", "bf16x3")


def trained_per_obj(sb, tb, per_obj):
    """Points per object the training operator launches: ragged objects are padded to whole wave tiles when there are latent terms."""
    return -(-per_obj // 32) * 32 if sb + tb > 0 and per_obj % 32 else per_obj


def e2e_cases():
    out = []
    for sb, tb in E2E_BLOCKS:
        for batch, (B, R, S) in BATCHES.items():
            split = split_takes(sb, tb, trained_per_obj(sb, tb, R * S))
            for prec in ["fp32", "bf16x3", TRIPLE, "auto"]:
                if prec in ("bf16x3", TRIPLE) and not split:
                    continue
                out.append((sb, tb, batch, prec))
    return out


def expected_run(sb, tb, precision, per_obj):
    """(forward, backward) arithmetic the training step must report in model.last_precision."""
    split = split_takes(sb, tb, trained_per_obj(sb, tb, per_obj))
    if precision == "auto":
        return ("bf16x3", "bf16x3") if split else ("fp32", "fp32")
    if precision == TRIPLE:
        return "fp32", "bf16x3"
    return precision, precision


@pytest.mark.parametrize("sb,tb,batch,precision", e2e_cases(), ids=lambda v: "-".join(v) if isinstance(v, tuple) else str(v))
def test_training_step_every_gradient(amd, dev, sb, tb, batch, precision):
    B, R, S = BATCHES[batch]
    per_obj = R * S
    params = O.init_decoder_params(sb, tb, seed=60 + sb + 10 * tb)
    g = torch.Generator().manual_seed(5 + sb + 10 * tb)
    xyz = torch.rand(B * R, S, 3, generator=g) * 2 - 1
    vd = F.normalize(torch.randn(B * R, 1, 3, generator=g), dim=-1).expand(B * R, S, 3).contiguous()
    sc0, tc0 = [torch.randn(B, 256, generator=g) * 0.3 for _ in range(2)]
    scale = (1.0 + torch.arange(B, dtype=torch.float32)).repeat_interleave(R)[:, None, None]
    ws, wr = torch.randn(B * R, S, 1, generator=g) * scale, torch.randn(B * R, S, 3, generator=g) * scale

    m = make_model(amd, dev, params, precision, (sb, tb), train=True)
    sc, tc = sc0.to(dev).requires_grad_(), tc0.to(dev).requires_grad_()
    sig, rgb = m(xyz.to(dev), vd.to(dev), sc, tc)
    fwd, bwd = expected_run(sb, tb, precision, per_obj)
    assert (m.last_precision["forward"], m.last_precision["backward"]) == (fwd, bwd), m.last_precision
    if precision == "auto" and sb + tb > 4:
        assert m.last_precision["forward"] == "fp32"
    masks = relu_bits_of(sig, sb, tb)
    ((sig * ws.to(dev)).sum() + (rgb * wr.to(dev)).sum()).backward()
    torch.cuda.synchronize()

    ref = {}
    for dt in (torch.float32, torch.float64):
        p = {k: v.detach().to(dt).clone().requires_grad_() for k, v in params.items()}
        s_, t_ = sc0.to(dt).clone().requires_grad_(), tc0.to(dt).clone().requires_grad_()
        s_o, r_o = O.decoder_forward(p, xyz.to(dt), vd.to(dt), s_, t_, relu_masks=masks)
        ((s_o * ws.to(dt)).sum() + (r_o * wr.to(dt)).sum()).backward()
        ref[dt] = {k: v.grad for k, v in p.items()}
        ref[dt].update(shape_code=s_.grad, texture_code=t_.grad)
    got = {k: v.grad for k, v in m.named_parameters()}
    got.update(shape_code=sc.grad, texture_code=tc.grad)
    assert sorted(got) == sorted(ref[torch.float64])
    for k, blocks in (("shape_code", sb), ("texture_code", tb)):
        if blocks == 0:             # no latent layer of this kind: nothing reaches the code
            assert ref[torch.float64][k] is None and (got[k] is None or not bool(got[k].any()))
            got.pop(k), ref[torch.float32].pop(k), ref[torch.float64].pop(k)
    check_all([(k, got[k], ref[torch.float32][k], ref[torch.float64][k]) for k in sorted(got)], bwd)


@pytest.mark.parametrize("sb,tb,precision", [(0, 0, "auto"), (5, 5, "fp32")])
def test_training_losses_and_bucket(amd, dev, sb, tb, precision):
    """trainer.nerf_losses into a GradBucket, as tests/test_driver_gpu.py::test_training_step_matches_oracle does at 3/1 blocks."""
    T = amd.trainer
    m = make_model(amd, dev, O.init_decoder_params(sb, tb, seed=80 + sb), precision, (sb, tb), train=True)
    codes = T.CodeTables(5, 256, seed=4).to(dev)
    g = torch.Generator().manual_seed(22)
    B, n, S = 2, 32, 64
    batch = dict(code_idx=torch.tensor([3, 1]), xyz=torch.rand(B, n, S, 3, generator=g) - 0.5,
                 viewdir=F.normalize(torch.randn(B, n, 1, 3, generator=g), dim=-1).repeat(1, 1, S, 1),
                 z_vals=torch.sort(torch.rand(B, S, generator=g) * 4 + 9, dim=-1)[0], rgb_tgt=torch.rand(B, n, 3, generator=g),
                 occ_pixels=(torch.randint(0, 3, (B, n, 1), generator=g) - 1).float())
    cpu_batch, batch = batch, {k: v.to(dev) for k, v in batch.items()}
    bucket = T.GradBucket(list(m.parameters()) + list(codes.parameters()))
    sc, tc = codes(batch["code_idx"])
    seen = {}

    def capturing(*a):
        out = m(*a)
        seen["masks"] = relu_bits_of(out[0], sb, tb)
        return out
    _, total = T.nerf_losses(capturing, batch["xyz"], batch["viewdir"], sc, tc, batch["z_vals"], batch["rgb_tgt"], batch["occ_pixels"], 0.1)
    total.backward()
    bucket.check_views()
    bwd = m.last_precision["backward"]
    assert bwd == ("bf16x3" if precision == "auto" and sb + tb <= 4 else "fp32"), m.last_precision
    ref = {}
    for dt in (torch.float32, torch.float64):
        p = {k: v.detach().cpu().to(dt).requires_grad_() for k, v in m.named_parameters()}
        w_sc = codes.shape_codes.weight.detach().cpu().to(dt).requires_grad_()
        w_tc = codes.texture_codes.weight.detach().cpu().to(dt).requires_grad_()
        b = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in cpu_batch.items()}
        with O.given_relu_masks(seen["masks"]):
            loss = O.training_losses(p, b["xyz"], b["viewdir"], w_sc[b["code_idx"]], w_tc[b["code_idx"]], b["z_vals"], b["rgb_tgt"],
                                     b["occ_pixels"], 0.1)[0]
        loss.backward()
        ref[dt] = {k: v.grad for k, v in p.items()}
        ref[dt].update(shape_codes=w_sc.grad, texture_codes=w_tc.grad)
    assert abs(float(total) - float(loss)) < 1e-5
    got = {k: v.grad for k, v in m.named_parameters()}
    got.update(shape_codes=codes.shape_codes.weight.grad, texture_codes=codes.texture_codes.weight.grad)
    if sb + tb == 0:
        for k in ("shape_codes", "texture_codes"):
            assert ref[torch.float64][k] is None and (got[k] is None or not bool(got[k].any()))
            got.pop(k), ref[torch.float32].pop(k), ref[torch.float64].pop(k)
    check_all([(k, got[k], ref[torch.float32][k], ref[torch.float64][k]) for k in sorted(got)], bwd)


# ------------------------------------------------------------------ c. one launch past 2^31 elements per dump
def test_large_launch_dumps_cross_2_31(amd, dev):
    """3/1 blocks, 2 objects x 599 264 points: P = 1 198 528, P % 128 = 64.  Slot 6 crosses element offset 2^31 at row 1 197 440 and slot 7
    lies entirely beyond it.  Sampled tiles against the taps, then every weight gradient against a float64 matmul of the same dumps."""
    ops = amd.ops
    sb, tb, B, n = 3, 1, 2, 599264
    P, n_slots = B * n, sb + tb + 4
    assert P % 128 == 64 and (6 * P + 1197440) * 256 == 2 ** 31 and 7 * P * 256 > 2 ** 31
    params = O.init_decoder_params(sb, tb, seed=90)
    ins = make_inputs(sb, tb, B, n, seed=91)
    tiles = [0, n // 32 - 1, n // 32, 1197440 // 32 - 1, 1197440 // 32, P // 32 - 1]
    rows = torch.cat([torch.arange(32 * t, 32 * t + 32) for t in tiles])
    obj = rows // n
    sample = (ins[0][rows], ins[1][rows], ins[2][obj], ins[3][rows], ins[4][rows])      # one object per sampled point
    torch.cuda.reset_peak_memory_stats(dev)
    for precision in ("fp32", "bf16x3"):
        xbuf, X, gbuf, G, masks = launch(amd, dev, params, sb, tb, *ins, precision)
        check_written(xbuf, X, "X")
        check_written(gbuf, G, "G")
        per_tile = (sb + tb + 3) * 64 * 16          # ReLU-bit bytes per 32-point tile (tests/relu_bits.py)
        sub = masks[: (P // 32) * per_tile].view(P // 32, per_tile)[torch.tensor(tiles, device=dev)].reshape(-1)
        ref = taps(params, *sample, decode_relu_bits(sub, rows.numel(), sb, tb))
        compare_dumps(X, G, ref, precision, rows=rows.to(dev), tag=f"{precision} ")

        pe = ops.pe_points(ins[0].to(dev), ins[1].to(dev))
        li_view = sb + 2
        pairs = []
        for li in range(n_slots):
            n_out = slot_width(li, n_slots)
            ops_in = [(pe[:, :64], 64)] if li == 0 else [(X[li - 1], 256)] + ([(pe[:, 64:], 28)] if li == li_view else [])
            Gl = G[li][:, :n_out]
            for k, (Xin, n_in) in enumerate(ops_in):
                dW, db = ops.weight_grad(Gl, n_out, Xin, n_in, precision=precision)
                Xv = Xin[:, :n_in]
                want64 = torch.zeros(n_out, n_in, dtype=torch.float64, device=dev)
                for r0 in range(0, P, 1 << 18):
                    want64 += Gl[r0:r0 + (1 << 18)].double().T @ Xv[r0:r0 + (1 << 18)].double()
                pairs.append((f"{precision} dW[{li}.{k}]", dW, Gl.T @ Xv, want64))
                if k == 0:
                    pairs.append((f"{precision} db[{li}]", db, Gl.sum(0), Gl.double().sum(0)))
        torch.cuda.synchronize()
        check_all(pairs, precision)
        del xbuf, X, gbuf, G, masks, pe, pairs
        torch.cuda.empty_cache()
    print(f"large launch: peak {torch.cuda.max_memory_allocated(dev) / 2 ** 30:.2f} GiB allocated")
