// Packed decoder-weight layout shared by host launchers and device kernels.
//
// The per-point layers of the decoder (src/model_supnerf.py:184-199 of the reference) are
// consumed by the fused kernels as a linear STREAM of k-chunks: one chunk = ROWS x 32 fp32,
// ROWS = output features of the layer (forward) or input features (backward, transposed
// weights), 32 = a slice of the reduction dimension.  Chunks are stored in exactly the
// order the kernel consumes them so the stream is read front to back with coalesced 16-byte
// LDS-DMA loads.  Reduction dimensions are zero-padded to a multiple of 32.  Inside a chunk the
// 16-byte slots of each row are XOR-swizzled (chunk_pos below).
#pragma once
#include <stdint.h>

#ifndef SNR_HD
#ifdef __HIPCC__
#define SNR_HD __host__ __device__
#else
#define SNR_HD
#endif
#endif

namespace snr {

constexpr int W = 256;           // hidden width == latent width
constexpr int W_RGB = 128;       // rgb.0 output width
constexpr int XYZ_FREQ = 10;
constexpr int DIR_FREQ = 4;
constexpr int D_XYZ = 3 + 6 * XYZ_FREQ;   // 63
constexpr int D_DIR = 3 + 6 * DIR_FREQ;   // 27
constexpr int KC = 32;           // reduction slice per chunk
constexpr int K_XYZ_PAD = 64;    // 63 -> 64
constexpr int K_VIEW_PAD = 288;  // 256 + 27 -> 288
constexpr int MAX_BLOCKS = 8;    // shape_blocks, texture_blocks <= 8

struct Layout {
    int sb, tb;
    int n_mfma_layers;   // sb + tb + 4 : enc_xyz, shape*sb, enc_shape, enc_viewdir, texture*tb, rgb0
    int n_lat;           // sb + tb
    // offsets in floats
    int64_t fwd;         // forward chunk stream
    int64_t bwd;         // backward (transposed) chunk stream
    int64_t bias;        // n_mfma_layers x 256
    int64_t sigma_w;     // 256
    int64_t sigma_b;     // 1 (padded to 4)
    int64_t rgb2_w;      // 3 x 128
    int64_t rgb2_b;      // 3 (padded to 4)
    int64_t bf_fwd;      // split-bf16 forward stream (offset in floats; contents are bf16 pairs)
    int64_t bf_bwd;      // split-bf16 backward stream
    int64_t total;       // floats
    int64_t fwd_floats, bwd_floats;
    int64_t bf_fwd_bytes, bf_bwd_bytes;
};

// ---- split-bf16 ("bf16x3") streams -------------------------------------------------------------------
// Every fp32 weight w is stored as hi = round16(w), lo = round16(w - hi) (fp16 in the forward stream, bf16 in the backward stream).  A chunk
// holds the weights of whole k32-steps as the exact LDS image the kernels read:
//   [k32-step s][16-row tile][plane hi/lo][lane 0..63][8 x 16 bit]          (1 KiB per (tile, plane): lane-linear)
// where element j of lane (n = lane&15, g = lane>>4) is W[row 16*tile + n][k = 32 s + 16 (j>>2) + 4 g + (j&3)] (backward: W^T) --
// the k order in which the 16x16 fp32 accumulator tiles 2s, 2s+1 re-enter v_mfma_f32_16x16x32_* as the B operand.
constexpr int BF_CHUNK = 32768;          // bytes of every chunk except the forward enc_viewdir ones
constexpr int BF_CHUNK_VIEW = 36864;     // 18 k16-steps

// ---- the layer table (host side) -----------------------------------------------------------------------
// The one description of the per-point layers.  Everything the packed buffer is made of follows from it: make_layout sums the per-layer
// sizes below, and the packers (snr_pack_weights, snr_bf16_pack_) walk the same table with the same size functions.  A layer's index
// (bias row, activation slot) is its place in `mfma`.  ops.decoder_layers is the Python twin (tests/test_host_logic.py ties the two).
struct Layer {
    int n_out, k_in;
    bool relu;
    int tensor;          // place of its (weight, bias) pair in snr_pack_weights' tensor list: reference order
};
struct LayerTable {
    int n;                                   // MFMA layers, in the order the kernels consume them
    Layer mfma[2 * MAX_BLOCKS + 4];
    Layer sigma, rgb2;                       // the two narrow heads (plain fp32 vectors behind the bias rows)
};
inline LayerTable layer_table(int sb, int tb) {
    LayerTable T;
    int n = 0, t = 0;
    T.mfma[n++] = {W, D_XYZ, true, t++};                                 // encoding_xyz
    for (int j = 0; j < sb; ++j) T.mfma[n++] = {W, W, true, t++};        // shape_layer_1..sb
    T.mfma[n++] = {W, W, false, t++};                                    // encoding_shape
    T.sigma = {1, W, false, t++};                                        // sigma.0
    T.mfma[n++] = {W, W + D_DIR, true, t++};                             // encoding_viewdir: hidden units, then the direction features
    for (int j = 0; j < tb; ++j) T.mfma[n++] = {W, W, true, t++};        // texture_layer_1..tb
    T.mfma[n++] = {W_RGB, W, true, t++};                                 // rgb.0
    T.rgb2 = {3, W_RGB, false, t++};                                     // rgb.2
    T.n = n;
    return T;
}

inline int k_pad(const Layer& l) { return (l.k_in + KC - 1) / KC * KC; }          // 64, 288 or 256
// fp32 streams: forward k_pad / KC chunks of n_out x KC floats, backward n_out / KC chunks of k_pad x KC floats -- n_out x k_pad either way
inline int64_t stream_floats(const Layer& l) { return (int64_t)l.n_out * k_pad(l); }
// split streams, 1 KiB per (tile, plane): forward n_out / 16 tiles x 2 planes per k32-step, backward 2 planes x n_out / KC steps per tile
// of 16 input features.  What lies past the hidden width (encoding_viewdir's direction features: forward step 8, backward tiles 16 and
// 17) is packed as a piece of its own behind the layer's other steps / tiles, hence the count argument.
inline int bf_fwd_steps(const Layer& l) { return k_pad(l) / KC; }
inline int bf_bwd_tiles(const Layer& l) { return (l.k_in + 15) / 16; }
inline int64_t bf_fwd_bytes(const Layer& l, int steps) { return (int64_t)(l.n_out / 16) * 2 * steps * 1024; }
inline int64_t bf_bwd_bytes(const Layer& l, int tiles) { return (int64_t)tiles * 2 * (l.n_out / KC) * 1024; }

inline Layout make_layout(int sb, int tb) {
    const LayerTable T = layer_table(sb, tb);
    Layout L;
    L.sb = sb; L.tb = tb;
    L.n_mfma_layers = T.n;
    L.n_lat = sb + tb;
    L.fwd_floats = L.bwd_floats = L.bf_fwd_bytes = L.bf_bwd_bytes = 0;
    for (int li = 0; li < T.n; ++li) {
        const Layer& l = T.mfma[li];
        L.fwd_floats += stream_floats(l);
        L.bwd_floats += stream_floats(l);
        L.bf_fwd_bytes += bf_fwd_bytes(l, bf_fwd_steps(l));
        L.bf_bwd_bytes += bf_bwd_bytes(l, bf_bwd_tiles(l));
    }
    int64_t o = 0;
    L.fwd = o; o += L.fwd_floats;
    L.bwd = o; o += L.bwd_floats;
    L.bias = o; o += (int64_t)T.n * W;
    L.sigma_w = o; o += T.sigma.n_out * T.sigma.k_in;
    L.sigma_b = o; o += 4;
    L.rgb2_w = o; o += T.rgb2.n_out * T.rgb2.k_in;
    L.rgb2_b = o; o += 4;
    o = (o + 3) & ~3ll;                       // 16-byte alignment for the LDS-DMA source
    L.bf_fwd = o; o += L.bf_fwd_bytes / 4;
    L.bf_bwd = o; o += L.bf_bwd_bytes / 4;
    L.total = o;
    return L;
}

// Position (in floats) of reduction column kk (0..31) of row `row` inside a chunk: the chunk is stored as
// the LDS image the kernels read, i.e. 16-byte slot c = kk/4 of a row sits at slot c ^ ((row >> 1) & 7).
// With 128-byte rows this makes every ds_read_b128 of a 32-row A fragment bank-conflict free (the 16
// lanes of a read group land on 16 distinct 16-byte slots of the 256-byte bank row) and lets the
// staging be a linear LDS-DMA copy.
SNR_HD inline int chunk_pos(int row, int kk) { return row * KC + ((((kk >> 2) ^ ((row >> 1) & 7)) << 2) | (kk & 3)); }

// ReLU masks saved by the forward pass for the backward pass: one bit per hidden unit of every
// ReLU layer, stored per 32-point wave tile as [layer][lane] uint4 (128 bits: the lane's 8 tiles x 16
// accumulator registers).  ReLU layers: enc_xyz, shape*sb, enc_viewdir, texture*tb, rgb0.
SNR_HD inline int n_relu_layers(int sb, int tb) { return sb + tb + 3; }
SNR_HD inline int64_t mask_bytes(int64_t n_points, int sb, int tb) {
    int64_t tiles = (n_points + 31) / 32;
    return tiles * n_relu_layers(sb, tb) * 64 * 16;
}

}  // namespace snr
