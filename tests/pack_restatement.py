"""Test helper: the packed decoder-weight buffer restated in numpy, from the description of the format (the comments of
csrc/snr_layout.h, and the kernel comments of csrc/snr_bf16.hip on the split image) and not from the packers.

The buffer, in floats and in this order (every float is defined; the scalar sections add up to a multiple of four floats, so the split
streams start 16-byte aligned without a gap):

  fwd      per MFMA layer in consumption order, ceil(k_in / 32) chunks of n_out rows x 32 floats: row = output feature, column kk of
           chunk c = input feature 32 c + kk, zero past k_in
  bwd      per MFMA layer in REVERSE order, n_out / 32 chunks of round_up(k_in, 32) rows x 32 floats: row = input feature (zero rows past
           k_in), column kk of chunk c = output feature 32 c + kk
           in both, the 16-byte slot s of a row sits at slot s ^ ((row >> 1) & 7)
  bias     one row of 256 per MFMA layer: the bias, then zeros (rgb.0 has 128 values)
  sigma_w  256          sigma_b  1 value, padded to 4          rgb2_w  3 x 128          rgb2_b  3 values, padded to 4
  bf_fwd   per MFMA layer in consumption order the image [k32-step][16-row tile][plane hi / lo][lane 0..63][8 x fp16]; element j of lane
           (n = lane & 15, g = lane >> 4) is W[16 tile + n][32 step + 16 (j >> 2) + 4 g + (j & 3)], zero past k_in; hi = rne(clamp(w, +-65504)),
           lo = rne(w - hi).  encoding_viewdir's direction step (k = 256 ..) is a piece of its own behind its eight others.
  bf_bwd   per MFMA layer in reverse order the same image of W^T in bf16: tile rows = input features, steps over the output features,
           hi = rne(w), lo = rne(w - hi), no clamp.  encoding_viewdir's tiles 16 and 17 (the direction features) are a piece of their own
           behind the sixteen others.

MFMA layers in consumption order: encoding_xyz, shape_layer_1..sb, encoding_shape, encoding_viewdir, texture_layer_1..tb, rgb.0."""
import numpy as np


def mfma_stems(sb, tb):
    return (["encoding_xyz.0"] + [f"shape_layer_{j}.0" for j in range(1, sb + 1)] + ["encoding_shape", "encoding_viewdir.0"]
            + [f"texture_layer_{j}.0" for j in range(1, tb + 1)] + ["rgb.0"])


def _up(n, m):
    return (n + m - 1) // m * m


def _padded(a, rows, cols):
    out = np.zeros((rows, cols), np.float32)
    out[:a.shape[0], :a.shape[1]] = a
    return out


def _swizzled(chunks):
    """(n_chunks, rows, 32) -> the same with every row's eight 16-byte slots at s ^ ((row >> 1) & 7)."""
    n, rows, _ = chunks.shape
    src = chunks.reshape(n, rows, 8, 4)
    out = np.empty_like(src)
    r = np.arange(rows)[:, None]
    out[:, r, np.arange(8)[None, :] ^ ((r >> 1) & 7)] = src
    return out.reshape(-1)


def fwd_chunks(w):
    n_out, k_in = w.shape
    kp = _up(k_in, 32)
    return _swizzled(_padded(w, n_out, kp).reshape(n_out, kp // 32, 32).transpose(1, 0, 2))


def bwd_chunks(w):
    n_out, k_in = w.shape
    kp = _up(k_in, 32)
    return _swizzled(_padded(w.T, kp, n_out).reshape(kp, n_out // 32, 32).transpose(1, 0, 2))


def _lane_image(m):
    """m (16 T, 32 S) -> [S][T][lane][8]: element j of lane (n, g) = m[16 t + n, 32 s + 16 (j >> 2) + 4 g + (j & 3)]."""
    T, S = m.shape[0] // 16, m.shape[1] // 32
    lane, j = np.arange(64)[:, None], np.arange(8)[None, :]
    kk = 16 * (j >> 2) + 4 * (lane >> 4) + (j & 3)
    return m.reshape(T, 16, S, 32).transpose(2, 0, 1, 3)[:, :, lane & 15, kk]


def _planes(hi, lo):
    """[S][T][lane][8] uint16 twice -> bytes of [S][T][plane][lane][8]."""
    return np.ascontiguousarray(np.stack([hi, lo], axis=2)).view(np.uint8).reshape(-1)


def _bf16_rne(x):
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def split_fwd(w):
    n_out, k_in = w.shape
    v = np.clip(_lane_image(_padded(w, n_out, _up(k_in, 32))), np.float32(-65504.0), np.float32(65504.0))
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    return _planes(hi.view(np.uint16), lo.view(np.uint16))      # step-major: a last step past the hidden width lands behind the others


def split_bwd(w):
    n_out, k_in = w.shape
    wt = _padded(w.T, _up(k_in, 16), n_out)
    pieces = []
    for rows in (wt[:256], wt[256:]):              # the hidden units' tiles, then (encoding_viewdir) the direction features' two
        if rows.shape[0]:
            v = _lane_image(rows)
            hi = _bf16_rne(v)
            lo = _bf16_rne(v - (hi.astype(np.uint32) << 16).view(np.float32))
            pieces.append(_planes(hi, lo))
    return np.concatenate(pieces)


def _f32_bytes(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint8)


def packed_sections(params, sb, tb):
    """[(section name, its bytes)] in buffer order; ``params``: numpy fp32 arrays under the reference's state-dict names."""
    stems = mfma_stems(sb, tb)
    ws = [params[s + ".weight"] for s in stems]
    bias = np.zeros((len(stems), 256), np.float32)
    for i, s in enumerate(stems):
        b = params[s + ".bias"]
        bias[i, :b.shape[0]] = b
    pad4 = lambda a: _padded(a[None, :], 1, 4)
    return [("fwd", _f32_bytes(np.concatenate([fwd_chunks(w) for w in ws]))),
            ("bwd", _f32_bytes(np.concatenate([bwd_chunks(w) for w in reversed(ws)]))),
            ("bias", _f32_bytes(bias)),
            ("sigma_w", _f32_bytes(params["sigma.0.weight"])), ("sigma_b", _f32_bytes(pad4(params["sigma.0.bias"]))),
            ("rgb2_w", _f32_bytes(params["rgb.2.weight"])), ("rgb2_b", _f32_bytes(pad4(params["rgb.2.bias"]))),
            ("bf_fwd", np.concatenate([split_fwd(w) for w in ws])),
            ("bf_bwd", np.concatenate([split_bwd(w) for w in reversed(ws)]))]


def packed_image(params, sb, tb):
    return np.concatenate([b for _, b in packed_sections(params, sb, tb)])


def zero_params(sb, tb):
    """A decoder of zeros in the reference's shapes (for size checks)."""
    shapes = {s: (256, 256) for s in mfma_stems(sb, tb)}
    shapes.update({"encoding_xyz.0": (256, 63), "encoding_viewdir.0": (256, 283), "rgb.0": (128, 256), "sigma.0": (1, 256), "rgb.2": (3, 128)})
    out = {}
    for s, (n_out, n_in) in shapes.items():
        out[s + ".weight"], out[s + ".bias"] = np.zeros((n_out, n_in), np.float32), np.zeros(n_out, np.float32)
    return out
