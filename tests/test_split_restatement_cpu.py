"""tests/split_restatement.py checked on the CPU: the chain against the oracle, the split model's error law on decoders rescaled by powers
of two (which scales the GPU tests of tests/test_decoder_range_gpu.py may use, and that a chip flushing fp16 subnormals would show), and
the numpy restatement of ``pe_sincos`` against float64 over the whole range of its fast branch."""
import numpy as np
import pytest
import torch

import split_restatement as R
from oracle import supnerf_oracle as O
from test_precision_guard import _points

RANGE_TOL = 1e-5            # ops.RANGE_TOL (asserted equal on the GPU side; the package needs its library to import)


def _inputs(P=512):
    xyz, vd, sc, tc = _points(torch.device("cpu"))
    return xyz.reshape(-1, 3)[:P].contiguous(), vd.reshape(-1, 3)[:P].contiguous(), sc, tc


@pytest.mark.parametrize("blocks", [(3, 1), (0, 0)])
def test_chain_is_the_oracle_in_float64(blocks):
    sb, tb = blocks
    params = {k: v.double() for k, v in O.init_decoder_params(sb, tb, seed=5 + sb).items()}
    g = torch.Generator().manual_seed(sb)
    B, n = 3, 40
    xyz = (torch.rand(B * n, 3, generator=g, dtype=torch.float64) - 0.5) * 2
    vd = torch.nn.functional.normalize(torch.randn(B * n, 3, generator=g, dtype=torch.float64), dim=-1)
    sc, tc = [torch.randn(B, 256, generator=g, dtype=torch.float64) * 0.3 for _ in range(2)]
    lat = O.latent_terms(params, sc, tc) if sb + tb else torch.zeros(B, 1, 256, dtype=torch.float64)
    sig_o, rgb_o = O.decoder_forward(params, xyz[:, None], vd[:, None], None, None, latent=lat)
    sig, rgb = R.decoder_chain(params, xyz, vd, lat, R.lin_exact(torch.float64))
    assert sig.dtype == torch.float64 and float((sig - sig_o.reshape(-1)).abs().max()) <= 1e-12
    assert float((rgb - rgb_o.reshape(-1, 3)).abs().max()) <= 1e-12


def test_fp16_pieces():
    """The pieces of the model: toward zero never grows a magnitude, keeps subnormals, and hi + lo carries 22 bits of a normal value."""
    x = torch.tensor([1.0, -1.0, 1.0 + 2.0 ** -16 + 2.0 ** -22, 65504.0, 1e6, -1e6, 2.0 ** -15, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 0.1, -0.1])
    hi, lo = R.split_pieces(x, toward_zero=True)
    xc = x.double().clamp(-65504, 65504)
    assert bool((hi.abs() <= xc.abs()).all()) and bool(((hi + lo).abs() <= xc.abs()).all())
    assert hi[4] == 65504.0 and hi[5] == -65504.0 and lo[4] == 0.0
    assert hi[6] == 2.0 ** -15 and hi[7] == 2.0 ** -24 and hi[8] == 0.0 and hi[9] == 2.0 ** -24          # subnormals kept, cut toward zero
    assert float(((hi + lo - xc).abs() / xc.abs())[[0, 1, 2, 3, 10, 11]].max()) <= 2.0 ** -21
    fh, fl = R.split_pieces(x, toward_zero=True, flush_subnormals=True)
    assert fh[6] == 0.0 and fh[7] == 0.0 and fh[0] == 1.0 and fl[2] == 0.0                                # a remainder below 2^-14: flushed
    nh, nl = R.split_pieces(torch.tensor([0.1, 1.0 + 3 * 2.0 ** -12]), toward_zero=False)
    assert float(nh[0]) == float(np.float32(np.float16(0.1))) and nh[1] == 1.0 + 2.0 ** -10              # nearest: up, where toward zero goes down


@pytest.fixture(scope="module")
def split_law(oracle_params):
    """{(how, k): (kept error, flushed error, fp32 chain error)} on the guard's points cut to 512, against the float64 chain of the SAME
    decoder; the float64 chain itself is unchanged by the rescaling (asserted)."""
    xyz, vd, sc, tc = _inputs()
    p64 = {n: v.double() for n, v in oracle_params.items()}
    base = R.decoder_chain(p64, xyz, vd, O.latent_terms(p64, sc.double(), tc.double()), R.lin_exact(torch.float64))
    out = {}
    for how in ("activations", "weights"):
        for k in (0, 4, 8, 12, 16, 20):
            params = R.scaled_decoder(oracle_params, how, k)
            q64 = {n: v.double() for n, v in params.items()}
            lat64 = O.latent_terms(q64, sc.double(), tc.double())
            want = R.decoder_chain(q64, xyz, vd, lat64, R.lin_exact(torch.float64))
            assert R.chain_error(want, base) <= 1e-12, (how, k)              # powers of two: the same function
            lat = O.latent_terms(params, sc, tc)
            out[how, k] = tuple(R.chain_error(R.decoder_chain(params, xyz, vd, lat, lin), want)
                                for lin in (R.lin_split_fp16(), R.lin_split_fp16(flush_subnormals=True), R.lin_exact(torch.float32)))
            print(f"[split law] {how:11s} 2^-{k:<2d}: kept {out[how, k][0]:.1e}  flushed {out[how, k][1]:.1e}  fp32 chain {out[how, k][2]:.1e}")
    return out


@pytest.mark.parametrize("how", ["activations", "weights"])
def test_split_error_law(split_law, how):
    """The split chain's error grows as 2^k: inside a quarter of the guard's tolerance at k = 4 and 8 (the guard must let such a decoder
    through), four tolerances and more at k = 16 and 20 (it must not).  The GPU tests use these scales only."""
    assert split_law[how, 0][0] <= RANGE_TOL / 4
    for k in (4, 8):
        assert split_law[how, k][0] <= RANGE_TOL / 4, (k, split_law[how, k])
    for k in (16, 20):
        assert split_law[how, k][0] >= 4 * RANGE_TOL, (k, split_law[how, k])
    for k in (0, 4, 8, 12, 16, 20):
        assert split_law[how, k][2] <= RANGE_TOL / 4, (k, split_law[how, k])   # the exact chain, the guard's reference, does not care


@pytest.mark.parametrize("how", ["activations", "weights"])
def test_flushed_model_is_far_worse(split_law, how):
    """What makes the GPU band (4 x the kept model's error) discriminating: at k = 4 a chain that flushed fp16 subnormals is 30 x worse."""
    kept, flushed, _ = split_law[how, 4]
    assert flushed >= 30 * kept, (kept, flushed)


# ------------------------------------------------------------------ pe_sincos
def _sincos_error(a):
    a = np.asarray(a, dtype=np.float32)
    sn, cs = R.pe_sincos_f32(a)
    a64 = a.astype(np.float64)
    return max(float(np.abs(sn.astype(np.float64) - np.sin(a64)).max()), float(np.abs(cs.astype(np.float64) - np.cos(a64)).max()))


def test_pe_sincos_restatement_over_the_fast_branch():
    """Max abs error against float64 sin / cos of the fp32 angle <= 1.0e-7 on every octave up to the seam at 8192, at every multiple of
    pi/2 (where the reduced argument is smallest and the quadrant changes) and across the seam into the library branch."""
    rng = np.random.default_rng(0)
    worst = {}
    for e in range(13):                                                      # [1, 2) .. [4096, 8192)
        mag = (2.0 ** e * (1.0 + rng.random(1_000_000))).astype(np.float32)
        worst[f"[{2 ** e}, {2 ** (e + 1)})"] = _sincos_error(np.concatenate([mag, -mag]))
    worst["below 1"] = _sincos_error((rng.random(1_000_000) * 2 - 1).astype(np.float32))
    k = np.arange(1, 5216, dtype=np.float64)
    mid = (k * (np.pi / 2)).astype(np.float32)
    assert float(mid.max()) <= 8192.0
    near = np.concatenate([mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(np.inf))])
    worst["k pi/2"] = _sincos_error(np.concatenate([near, -near]))
    seam = np.float32(8192.0)
    edge = np.array([seam, np.nextafter(seam, np.float32(0)), np.nextafter(seam, np.float32(np.inf))], dtype=np.float32)
    worst["seam"] = _sincos_error(np.concatenate([edge, -edge]))
    for name, err in worst.items():
        print(f"[pe_sincos restated] {name}: {err:.2e}")
    assert max(worst.values()) <= 1.0e-7, worst
