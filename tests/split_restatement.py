"""Test helper (CPU; torch + numpy only): the decoder's per-point chain restated with a pluggable linear, a model of the split forward's
fp16 pieces, decoders rescaled by powers of two, and the encodings' sin / cos restated in numpy.

``decoder_chain`` follows the kernels' dataflow (csrc/snr_mlp.hip, csrc/snr_bf16.hip): every 256-wide layer goes through ``lin(x, W, b)``,
the latent term is added AFTER the ReLU, the density head reads encoding_shape's output, and the two narrow heads (sigma.0, rgb.2) are
plain products in the chain's working precision.  With ``lin_exact(torch.float64)`` it is ``oracle.decoder_forward(..., latent=...)``.

``lin_split_fp16`` models one layer of the split forward: the activation clamped to +-65504 and cut into hi = fp16 toward zero
and lo = fp16 toward zero of the remainder (v_cvt_pkrtz and the v_fma_mix remainder); the weight clamped and cut with round-to-nearest
for both pieces (pack_bf16_kernel's forward branch); the three products hi hi + hi lo + lo hi exact, summed in float64 on the bias and rounded
to fp32 once.  fp16 subnormals are KEPT -- ``flush_subnormals=True`` zeroes every piece below 2^-14 instead, which is what the chip must not
be doing: on a decoder whose activations or weights are small the two models part by orders of magnitude (tests/test_split_restatement_cpu.py),
and the kernels are held to the first one (tests/test_decoder_range_gpu.py)."""
import numpy as np
import torch

from oracle import supnerf_oracle as O

FP16_MAX = 65504.0
FP16_MIN_NORMAL = 2.0 ** -14


# ------------------------------------------------------------------ fp16 pieces
def _fp16_toward_zero(x32: np.ndarray) -> np.ndarray:
    """fp32 -> fp16 rounded toward zero (subnormals kept), returned as fp32.  |x| <= 65504."""
    h = x32.astype(np.float16)                                   # round to nearest even ...
    over = np.abs(h.astype(np.float32)) > np.abs(x32)            # ... and one step back where that went away from zero
    h = np.where(over, np.nextafter(h, np.float16(0.0)), h)
    return h.astype(np.float32)


def _fp16_nearest(x32: np.ndarray) -> np.ndarray:
    return x32.astype(np.float16).astype(np.float32)


def split_pieces(x: torch.Tensor, toward_zero: bool, flush_subnormals: bool = False):
    """(hi, lo) float64 tensors: the two fp16 pieces of the fp32 values ``x`` after the clamp to +-65504."""
    x32 = np.clip(x.detach().to(torch.float32).numpy(), -FP16_MAX, FP16_MAX).astype(np.float32)
    cut = _fp16_toward_zero if toward_zero else _fp16_nearest
    hi = cut(x32)
    lo = cut((x32 - hi).astype(np.float32))                      # the remainder is exact in fp32
    if flush_subnormals:
        hi = np.where(np.abs(hi) < FP16_MIN_NORMAL, np.float32(0.0), hi)
        lo = np.where(np.abs(lo) < FP16_MIN_NORMAL, np.float32(0.0), lo)
    return torch.from_numpy(hi.astype(np.float64)), torch.from_numpy(lo.astype(np.float64))


# ------------------------------------------------------------------ linears
class lin_exact:
    """The plain linear in ``dtype``; the chain then works in ``dtype`` throughout."""

    def __init__(self, dtype):
        self.dtype = dtype

    def __call__(self, x, W, b):
        return torch.nn.functional.linear(x.to(self.dtype), W.to(self.dtype), b.to(self.dtype))


class lin_split_fp16:
    """One layer of the split forward (module docstring); the chain works in fp32 between the layers."""
    dtype = torch.float32

    def __init__(self, flush_subnormals=False):
        self.flush = flush_subnormals
        self._weights = {}

    def __call__(self, x, W, b):
        key = id(W)
        if key not in self._weights:                             # (a weight is cut once, like the packed stream)
            self._weights[key] = (W, split_pieces(W, toward_zero=False, flush_subnormals=self.flush))
        w_hi, w_lo = self._weights[key][1]
        x_hi, x_lo = split_pieces(x, toward_zero=True, flush_subnormals=self.flush)
        acc = x_hi @ w_hi.t() + x_hi @ w_lo.t() + x_lo @ w_hi.t() + b.detach().double()
        return acc.to(torch.float32)


# ------------------------------------------------------------------ the chain
def _pe(x, degree, dtype):
    """The positional encoding from float64 sin / cos of the exact angles, rounded to the chain's precision."""
    return O.positional_encoding(x.double(), degree).to(dtype)


def decoder_chain(params, xyz, viewdir, latent, lin, zeroed=None):
    """(sigma (P,), rgb (P,3)) of points ``xyz``, ``viewdir`` (P,3) and latent terms ``latent`` (B, NLAT, 256), object-major with P / B points
    each, every 256-wide layer through ``lin``.  ``zeroed``: {layer name: boolean (P,) mask} of points whose output of that ReLU layer
    (after the ReLU, before the latent term) is forced to 0 -- what a ReLU that erases a NaN leaves behind."""
    dt = lin.dtype
    sb, tb = O._count_blocks(params)
    P, B = xyz.shape[0], latent.shape[0]
    rows = lambda j: latent[:, j].to(dt).repeat_interleave(P // B, dim=0)
    layer = lambda name, t: lin(t, params[name + ".weight"], params[name + ".bias"])
    head = lambda name, t: torch.nn.functional.linear(t, params[name + ".weight"].to(dt), params[name + ".bias"].to(dt))

    def relu_layer(name, t):
        y = torch.relu(layer(name, t))
        if zeroed is not None and name in zeroed:
            y = torch.where(zeroed[name][:, None], torch.zeros_like(y), y)
        return y

    h = relu_layer("encoding_xyz.0", _pe(xyz, 10, dt))
    for j in range(1, sb + 1):
        h = relu_layer(f"shape_layer_{j}.0", h + rows(j - 1))
    h = layer("encoding_shape", h)
    sigma = torch.nn.functional.softplus(head("sigma.0", h))
    h = relu_layer("encoding_viewdir.0", torch.cat([h, _pe(viewdir, 4, dt)], dim=-1))
    for j in range(1, tb + 1):
        h = relu_layer(f"texture_layer_{j}.0", h + rows(sb + j - 1))
    rgb = head("rgb.2", relu_layer("rgb.0", h))
    return sigma.reshape(P), rgb.reshape(P, 3)


def chain_error(got, want):
    """max |got - want| / max(1, |want|) over sigma and rgb: the measure of ops.outputs_disagree."""
    return max(float(((g.double().cpu() - w.double()).abs() / w.double().abs().clamp_min(1.0)).max()) for g, w in zip(got, want))


# ------------------------------------------------------------------ decoders rescaled by powers of two
SCALED = {"activations": ("encoding_xyz.0", "shape_latent_layer_1.0", "shape_layer_1.0"),
          "weights": ("shape_layer_2.0", "shape_latent_layer_3.0", "shape_layer_3.0")}


def scaled_decoder(params, how, k):
    """A copy of ``params`` (3 shape blocks at least) computing the same function with one stretch of the chain 2^-k times smaller:
    ``how="activations"``: encoding_xyz.0 (weight and bias) and latent row 0 (its latent layer's weight and bias: the ReLU is
    homogeneous) times 2^-k, shape_layer_1.0.weight times 2^k; ``how="weights"``: the same across shape_layer_2.0 / shape_layer_3.0 with
    latent row 2.  Powers of two: every scaled tensor is exact, and in exact arithmetic the function is unchanged."""
    small, latent_layer, undo = SCALED[how]
    s = 2.0 ** -k
    out = {n: v.clone() for n, v in params.items()}
    for n in (small, latent_layer):
        out[n + ".weight"] *= s
        out[n + ".bias"] *= s
    out[undo + ".weight"] /= s
    return out


# ------------------------------------------------------------------ the encodings' sin / cos
def _fma(a, b, c):
    """fmaf on fp32 arrays: one rounding of the float64 product-sum (the product of two fp32 values is exact in float64)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


PE_FAST_LIMIT = 8192.0


def pe_sincos_f32(a):
    """(sin, cos) of the fp32 angles ``a`` as ``pe_sincos`` (csrc/snr_device.hpp) computes them: the same constants in the same order up
    to |a| <= 8192, the library branch beyond as float64 sin / cos of the angle rounded to fp32."""
    f = np.float32
    a = np.asarray(a, dtype=np.float32)
    k = np.rint(a * f(0.636619772367581343))
    r = _fma(-k, np.full_like(a, f(1.57079637050628662109375)), a)
    r = _fma(-k, np.full_like(a, f(-4.371138828673793e-8)), r)
    r = _fma(-k, np.full_like(a, f(-1.7763568394002505e-15)), r)
    z = r * r
    one = np.ones_like(a)
    ps = _fma(_fma(one * f(-1.9515295891e-4), z, one * f(8.3321608736e-3)), z, one * f(-1.6666654611e-1))
    s = _fma(ps * z, r, r)
    pc = _fma(_fma(one * f(2.443315711809948e-5), z, one * f(-1.388731625493765e-3)), z, one * f(4.166664568298827e-2))
    c = _fma(pc * z, z, _fma(one * f(-0.5), z, one))
    fast = np.abs(a) <= f(PE_FAST_LIMIT)
    q = np.where(fast, k, 0).astype(np.int64)
    s1, c1 = np.where(q & 1, c, s), np.where(q & 1, s, c)
    sn, cs = np.where(q & 2, -s1, s1), np.where((q + 1) & 2, -c1, c1)
    a64 = a.astype(np.float64)
    return (np.where(fast, sn, np.sin(a64).astype(np.float32)).astype(np.float32),
            np.where(fast, cs, np.cos(a64).astype(np.float32)).astype(np.float32))
