// Fused decoder forward for gfx950, exact fp32, TWO waves per SIMD: v_mfma_f32_16x16x4_f32 on 16 points per wave.
//
// Same path as snr_mlp.hip (positional encoding -> code-conditioned MLP on the fp32 MFMA pipe -> optional alpha composite, one
// launch), same packed weight stream, same LDS map, same outputs and ReLU-bit layout.  What differs is the shape of the work:
//
//   * Workgroup = 8 waves = 128 consecutive sample points; wave w owns points 16 w .. 16 w + 15, TWO waves share a SIMD
//     (__launch_bounds__(512, 2): at most 256 registers each).  The matrix pipe is per SIMD: whatever one wave does between its
//     MFMAs -- bias into the accumulators, ReLU / latent add / ReLU bits of the previous layer, the density and colour heads, LDS
//     waits -- runs while the partner wave's MFMAs keep the pipe busy.  With one 512-register wave per SIMD (snr_mlp.hip) that work
//     was exposed: 7.6 % of the kernel at the layer boundaries, which five ways of hiding under the wave's OWN MFMAs did not recover
//     (tools/_diag/experiments/README.md).
//   * GEMMs transposed as before, Y^T = W X^T: the weight slice is the A operand, the wave's 16 points the B / C / D columns.
//     v_mfma_f32_16x16x4_f32 (32 cycles, 64 FLOP/clk/SIMD like 32x32x2): accumulator register r of lane (n = lane & 15, g = lane >> 4)
//     of tile T holds feature 16 T + 4 g + r of point n -- which is the B operand of the NEXT layer's k-slice {16 T + 4 g' + r : g'}
//     when the matching A fragment (row m = lane & 15, k = 16 T + 4 g .. + 3) is fetched with ONE ds_read_b128: the accumulators of
//     layer l are the B operands of layer l + 1 with no data movement, as in the 32x32 kernel.  That fragment is 16 consecutive bytes
//     of the EXISTING packed image (row-major 128-byte rows, 16-byte slots XOR-swizzled by (row >> 1) & 7) and the 64 lanes' reads are
//     bank-conflict free on it (checked for all four ds_read_b128 lane groups), so snr_pack_weights is unchanged.
//   * Layers run k-outer over the previous layer's tiles: input tile T of layer l + 1 is made from accumulator tile T of layer l
//     (ReLU, latent add, ReLU bits) just before its 64 MFMAs; two accumulator sets (previous layer's
//     values, current sums: 64 + 64 registers), the last k-step deposits the finished tiles in the dead previous set.
//   * One 32 KiB weight chunk (32 k) = two input tiles = 128 MFMAs per wave; ring of two buffers, one barrier per chunk as before.
//
// The fma chain of an output differs from the 32x32x2 kernel's in the ORDER of the k terms (a 16x16x4 MFMA sums k = 16 T + {r, 4 + r,
// 8 + r, 12 + r}, the 32x32x2 form k = 32 c + 8 j + {e, 4 + e}): both are exact fp32 fma chains over the same products, results agree
// to fp32 round-off, not bit for bit.
#include <atomic>
#include <type_traits>

#include "snr_mlp16_core.hpp"
#include "snr_host.hpp"

namespace snr {

// What happens to a finished accumulator tile of the PREVIOUS layer on its way into the current layer's B operand.
struct Epi {
    float lo;                 // ReLU floor: 0, or -inf for the layer without an activation
    const float* zlds;        // LATLDS: LDS row of the latent term added after the activation (the zero row if none)
    const float* zglb;        // !LATLDS: this lane's global latent row, or null
    float hi;                 // +inf, opaque (made once per kernel): the upper bound of the ReLU's v_med3
};
struct EpiRegs { f32x4 z; };          // what a tile's epilogue reads from LDS, requested a tile ahead

__device__ __forceinline__ uint32_t spread_nibbles(uint32_t m16) {
    // nibble of input tile dT (shifted in first = highest) -> bits 8 dT .. 8 dT + 3
    return ((m16 >> 12) & 0xFu) | (((m16 >> 8) & 0xFu) << 8) | (((m16 >> 4) & 0xFu) << 16) | ((m16 & 0xFu) << 24);
}

template <bool LATLDS>
__device__ __forceinline__ EpiRegs epi_load(const Epi& c, int T, int g) {
    EpiRegs e;
    e.z = f32x4{0.f, 0.f, 0.f, 0.f};
    if (LATLDS) e.z = *reinterpret_cast<const f32x4*>(c.zlds + 16 * T + 4 * g);
    else if (c.zglb) e.z = *reinterpret_cast<const f32x4*>(c.zglb + 16 * T + 4 * g);
    return e;
}

// one value of accumulator tile T of the previous layer -> B-operand register r of input tile T (feature 16 T + 4 g + r): ReLU (or none),
// ReLU bit (shifted in: call with r = 3, 2, 1, 0), the density head's term, the latent add.  Five VALU instructions, placed by the caller
// BETWEEN the MFMA groups of the tile before (see layer_from_acc).
template <bool MASKS>
__device__ __forceinline__ void epi_value(const f32x4& acc, f32x4& x, const Epi& c, const EpiRegs& e, int r, uint32_t& m16) {
    float v = acc[r];
    if (MASKS) m16 = __builtin_amdgcn_alignbit(m16, __float_as_uint(0.f - v), 31);      // bit = (v > 0): the sign of 0 - v (+0 and -0 give 0)
    v = __builtin_amdgcn_fmed3f(v, c.lo, c.hi);
    x[r] = v + e.z[r];
    if (MASKS) asm volatile("" : "+v"(m16));      // (pinned: left alone the compiler sinks the bit collection to the end of the layer)
}

template <int NT>
__device__ __forceinline__ void acc_from_bias(f32x4 (&acc)[16], const float* bias /* LDS, layer's row */, int g) {
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = *reinterpret_cast<const f32x4*>(bias + 16 * t + 4 * g);
}

// One layer whose K = 256 inputs are the previous layer's accumulators accP: NT output tiles (16: 256 rows; 8: rgb.0), chunks
// base + 0 .. 7 of the stream.  `pre` (uniform; enc_viewdir): the layer also has a chunk of explicit operand tiles xe (the direction
// features) -- chunk 8 of its stream, consumed FIRST, so that the last MFMA step of every layer is the same deposit into accP (with the
// extra chunk behind the eight, the merge of the two ends of the layer cost 48 spilled registers).  On entry the layer's first chunk
// (the direction chunk if `pre`) is in the current buffer and its first fragment pair is requested into (a0, a1); at its last chunk the
// layer requests `next_first` (next_rows rows; 0 = the stream ends) and, with the rendezvous taken inside the chunk's last MFMA group
// (RingTurn), that chunk's first fragment pair: the pair is carried from chunk to chunk and from layer to layer.  Only the direction
// chunk keeps the rendezvous behind its MFMAs.  On return accP holds this layer's sums (bias included, no activation yet).
// RAY (the fused render's instantiations) and `ray` (uniform: the workgroup is one ray): the direction chunk is summed once per workgroup,
// see below; the layer BEFORE that one passes next_off = own_rows16 so that the pair it hands on is the wave's own.
template <int NT, int WAVES, bool LATLDS, bool MASKS, bool RAY = false>
__device__ __forceinline__ void layer_from_acc(f32x4 (&accP)[16], Ring16& ring, float* lds, const float* bias, const Epi& c, int g, const Dma16& dm,
                                               const float* base, bool pre, const f32x4 (&xe)[2], const float* next_first, int next_rows,
                                               uint32_t (&mw)[4], f32x4& a0, f32x4& a1, bool ray = false, int next_off = 0) {
    f32x4 accC[16];
    constexpr int rows_mid = NT * 16;
    constexpr int chunk_floats = rows_mid * KC;
    if (pre) {
        chunk_dma16<WAVES>(dm, base, lds + (ring.cur ^ 1) * WBUF16, lds, rows_mid);
        const bool once = RAY && NT == 16 && ray;
        if (once) {
            // The direction chunk when the workgroup is ONE ray (fused render, S = 16 WAVES): every column of every wave holds the same B
            // operands xe, so the chunk's 256 sums are the same in all 16 WAVES columns -- computed once, by the workgroup together.  Wave w
            // takes output tiles NTW w .. NTW w + NTW - 1 (NTW = 16 / WAVES): bias, xe[0]'s four k-steps, xe[1]'s four, the MFMAs the full form
            // issues for those tiles on the same A fragments (rows 16 NTW w .. of the chunk: own_rows16; the pair carried in is already that
            // wave's own, the layer before requested it at next_off) in the same order; column 0 (n = 0, one lane per g) writes the tile
            // back IN PLACE into the layer's bias row, slot 16 t + 4 g: the layout acc_from_bias reads, as a broadcast over n.  Behind the
            // chunk's rendezvous every wave starts its accumulators from that row and goes on with the 256 features as before.
            //   * Bit for bit the full form's sums: an MFMA's column n depends on column n of B and C alone; B is the same in all columns
            //     and C (the bias) is a broadcast over n, so column 0 of the tile IS every column of it -- the same instruction on the same
            //     operand bits, NaN and infinite directions included.  The chain per output stays bias, xe[0], xe[1], then the eight chunks.
            //   * Before the barrier a wave reads and writes only ITS tiles' slots of the row; the writes are complete (lgkmcnt(0)) when it
            //     arrives, so behind the barrier every wave reads finished sums.  Nobody needs the plain biases again: the row is restaged
            //     by every workgroup's prologue, and enc_viewdir is consumed once.
            //   * No LDS, barrier or DMA the full form does not have; the accumulator start is the same 16 ds_read_b128, behind the barrier.
            constexpr int NTW = 16 / WAVES;
            const float* wb = lds + ring.cur * WBUF16 + own_rows16<WAVES>(dm);
            float* own = const_cast<float*>(bias) + dm.wave * (NTW * 16) + 4 * g;
            f32x4 accS[NTW];
#pragma unroll
            for (int t = 0; t < NTW; ++t) accS[t] = *reinterpret_cast<const f32x4*>(own + 16 * t);
            tile_mma<NTW, 0, NoBetween, NoTurn, NTW>(accS, accP, xe[0], wb + ring.aoff[0], a0, a1, wb + ring.aoff[1]);
            tile_mma<NTW, 0, NoBetween, NoTurn, NTW>(accS, accP, xe[1], wb + ring.aoff[1], a0, a1, nullptr);
            if ((threadIdx.x & 15) == 0) {
#pragma unroll
                for (int t = 0; t < NTW; ++t) *reinterpret_cast<f32x4*>(own + 16 * t) = accS[t];
            }
            SNR16_WAIT_LDS();
        } else {
            const float* wb = lds + ring.cur * WBUF16;
            acc_from_bias<NT>(accC, bias, g);
            tile_mma<NT, false>(accC, accP, xe[0], wb + ring.aoff[0], a0, a1, wb + ring.aoff[1]);
            tile_mma<NT, false>(accC, accP, xe[1], wb + ring.aoff[1], a0, a1, nullptr);
        }
        ring_turn(ring);
        if (once) acc_from_bias<NT>(accC, bias, g);
        first_pair(a0, a1, lds + ring.cur * WBUF16 + ring.aoff[0]);
    } else {
        acc_from_bias<NT>(accC, bias, g);
    }
    // Input tile T's four operand registers are made from accP[T] while tile T - 1's MFMAs run: one value (five VALU instructions) behind
    // every second MFMA group of that tile, its latent / head-weight rows requested behind the first group; the LDS-DMA pieces of the next
    // chunk go out one per group as well.  Nothing but the tile's own MFMAs then stands between two tiles -- with the previous form (whole
    // epilogue + four DMA pieces at the top of a tile) both waves of a SIMD, which run this program in lockstep, left the matrix pipe idle
    // together.  Only the layer's first tile is made up front.
    constexpr int NG = NT / 2;                   // MFMA groups per tile
    EpiRegs e = epi_load<LATLDS>(c, 0, g);
    f32x4 xa, xb;
    uint32_t m16 = 0u;
#pragma unroll
    for (int r = 3; r >= 0; --r) epi_value<MASKS>(accP[0], xa, c, e, r, m16);
#pragma unroll
    for (int ch = 0; ch < 8; ++ch) {
        const float* src = (ch < 7) ? base + (ch + 1) * chunk_floats : next_first;
        const int rows = (ch < 7) ? rows_mid : next_rows;
        float* const dst = lds + (ring.cur ^ 1) * WBUF16;
        const float* wb = lds + ring.cur * WBUF16;
        // the next chunk's first fragment pair, requested behind the early rendezvous.  The 256-row layers always have a successor in the
        // full forward; in the density-only modes enc_shape's last chunk requests a pair nobody uses from a buffer nobody writes again.
        const float* const wn = (ch < 7 || NT == 16) ? dst + ring.aoff[0] + ((RAY && ch == 7) ? next_off : 0) : nullptr;
        // first tile of the chunk (T = 2 ch) on xa; between its groups: the next chunk's DMA pieces and tile 2 ch + 1's operand
        tile_mma<NT, false>(accC, accP, xa, wb + ring.aoff[0], a0, a1, wb + ring.aoff[1], [&](int gi) {
            if (gi == 0) e = epi_load<LATLDS>(c, 2 * ch + 1, g);
            constexpr int PSTEP = (WAVES == 8) ? 2 : 1;      // a piece covers 8 WAVES rows: 4 (8 waves) or 8 (4 waves) pieces per 256-row chunk
            if (gi % PSTEP == 0 && (gi / PSTEP) * 8 * WAVES < rows) chunk_piece16<WAVES>(dm, src, dst, lds, rows, gi / PSTEP);
#pragma unroll
            for (int k = (gi * 4) / NG; k < ((gi + 1) * 4) / NG; ++k) epi_value<MASKS>(accP[2 * ch + 1], xb, c, e, 3 - k, m16);
        });
        if (ch & 1) { mw[ch >> 1] = m16; m16 = 0u; }
        // second tile (T = 2 ch + 1) on xb; between its groups: tile 2 ch + 2's operand (the next chunk's first tile)
        if (ch == 7) {
            tile_mma<NT, true>(accC, accP, xb, wb + ring.aoff[1], a0, a1, wn, NoBetween(), RingTurn());
        } else {
            tile_mma<NT, false>(accC, accP, xb, wb + ring.aoff[1], a0, a1, wn, [&](int gi) {
                if (gi == 0) e = epi_load<LATLDS>(c, 2 * ch + 2, g);
#pragma unroll
                for (int k = (gi * 4) / NG; k < ((gi + 1) * 4) / NG; ++k) epi_value<MASKS>(accP[2 * ch + 2], xa, c, e, 3 - k, m16);
            }, RingTurn());
        }
        ring.cur ^= 1;
    }
}

// the lane's 64 ReLU bits of a layer (4 words x 16 bits: nibbles of input tiles 4 w .. 4 w + 3) -> the documented layout (snr_layout.h: per
// 32-point tile [layer][lane (p, h)] uint4, word w bit 16 (t & 1) + 4 j + e <-> feature 32 t + 8 j + 4 h + e) and stored.  Feature 16 T + 4 g + r
// is bit 8 (T & 3) + 4 (g >> 1) + r of word T >> 2 of lane (p, h = g & 1): lanes g and g ^ 2 (= lane ^ 32) hold the two nibble columns.
__device__ __forceinline__ void store_masks16x4(uint4* __restrict__ dst /* tile's [64] uint4 of this layer */, const uint32_t (&mw)[4], int wave, int lane) {
    const int n = lane & 15, g = lane >> 4;
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t mine = spread_nibbles(mw[i]) << (4 * (g >> 1));
        w[i] = mine | (uint32_t)__shfl_xor((int)mine, 32, 64);
    }
    if (g < 2) dst[16 * (wave & 1) + n + 32 * g] = make_uint4(w[0], w[1], w[2], w[3]);
}

#ifdef SNR_STAMPS   /* diagnostic build (tools/build_diag.sh): lane 0 of every wave writes s_memtime at phase boundaries into the sigmas buffer, 8 per
                       16-point wave tile (tools/_diag/stamps16.py prints them); the renders of such a build are valid, the saved sigmas are not */
#define SNR16_STAMP(i) do { if (io.sigmas && lane == 0) { unsigned long long t_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); \
        reinterpret_cast<unsigned long long*>(io.sigmas)[(tile_wg * WAVES + wave) * 8 + (i)] = t_; } } while (0)
/* slot 6 takes the wave's place on the chip instead: HW_ID (wave, SIMD, CU, SE) | XCC_ID << 32 */
#define SNR16_STAMP_HWID(i) do { if (io.sigmas && lane == 0) { unsigned a_, b_; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)\n\ts_getreg_b32 %1, hwreg(HW_REG_XCC_ID)" : "=s"(a_), "=s"(b_)); \
        reinterpret_cast<unsigned long long*>(io.sigmas)[(tile_wg * WAVES + wave) * 8 + (i)] = (unsigned long long)a_ | ((unsigned long long)b_ << 32); } } while (0)
#else
#define SNR16_STAMP(i) do {} while (0)
#define SNR16_STAMP_HWID(i) do {} while (0)
#endif

// the kernel argument that says where a launch's points come from (the modes: snr_host.hpp)
template <int MODE> struct PointSrc { using T = RayGeom; };
template <> struct PointSrc<MODE_LATTICE> { using T = snr_lattice; };
template <> struct PointSrc<MODE_BRICKS> { using T = BrickSrc; };

// MODE 0: explicit points; 1: fused render; 2 and 3: density only (explicit points; points of a lattice, object-major, x-major / z fastest):
// the same chain up to the density head -- same instructions, so the same sigma bit for bit -- and nothing after it: no view direction, no
// enc_viewdir / texture / rgb layers.  The stream's last request is then enc_shape's last chunk.  With MASKS (mode 2 only: snr_density_fwd_masks)
// the ReLU bits of enc_xyz and the shape layers go to their slots of the full forward's layout; the texture-branch slots are not written.
// MODE 4: density only on listed bricks of a lattice (snr_density_bricks): 512 points per brick, so every workgroup (64 or 128 points) lies in
// one brick and belongs to that brick's object; mode 3's coordinates, a scattered store into the (B, n0, n1, n2) grid.
template <int MODE, int WAVES, bool LATLDS, bool MASKS>
__global__ void __launch_bounds__(WAVES * 64, 2)
decoder_fwd16_kernel(DecoderIO io, Layout L, Lds16 lo, const float* __restrict__ xyz, const float* __restrict__ viewdir, typename PointSrc<MODE>::T gm,
                     float* __restrict__ out_rgb, float* __restrict__ out_depth, float* __restrict__ out_acc) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int WGP = WAVES * 16;                      // points per workgroup
    constexpr bool DENS = MODE >= 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 15, g = lane >> 4;
    const long long tile_wg = blockIdx.x;
    const long long gp_raw = tile_wg * WGP + wave * 16 + n;
    const bool live = gp_raw < io.n_points;
    const long long gp = live ? gp_raw : io.n_points - 1;
    const long long tile32 = tile_wg * (WAVES / 2) + (wave >> 1);
    const bool tile_live = tile32 * 32 < io.n_points;
    const int sb = io.sb, tb = io.tb;
    const int n_relu = n_relu_layers(sb, tb);
    SNR16_STAMP(0);
    // The prologue and the tail are VALU work; the SIMD's other wave (another workgroup, out of phase) is mid-stream, issuing MFMAs back to back,
    // and at equal priority its ready MFMA wins the ALUs nearly every time: the prologue then takes 69 000 cycles instead of 9 000 and the matrix
    // pipe is fed by one wave (0.87 of its rate) for that long.  With priority the prologue is over in a fraction of that and two waves share
    // the pipe again (tools/_diag/stamps16.py).
    __builtin_amdgcn_s_setprio(3);
    float px, py, pz, dx, dy, dz, zc = 0.f;
    long long b_obj = 0, b_dst = 0;          // mode 4: the brick's object, where the lane's sigma goes
    bool b_keep = false;                     // mode 4: the lane's point lies in the grid (and its brick in range)
    if constexpr (MODE == 0) {
        px = xyz[gp * 3]; py = xyz[gp * 3 + 1]; pz = xyz[gp * 3 + 2];
        dx = viewdir[gp * 3]; dy = viewdir[gp * 3 + 1]; dz = viewdir[gp * 3 + 2];
    } else if constexpr (MODE == 1) {
        const PointId id = point_id(gm, tile_wg, WGP, wave * 16 + n, live);
        const SamplePoint sp = make_sample(gm, id.ray, id.s, id.obj);
        px = sp.x; py = sp.y; pz = sp.z; dx = sp.dx; dy = sp.dy; dz = sp.dz; zc = sp.zc;
    } else if constexpr (MODE == 2) {
        px = xyz[gp * 3]; py = xyz[gp * 3 + 1]; pz = xyz[gp * 3 + 2];
        dx = dy = dz = 0.f;
    } else if constexpr (MODE == 3) {
        // lattice point (i, j, k) of the lane's object: lo + h * i per axis, one multiply and one add (the library builds with -ffp-contract=off)
        const long long obj = gp / io.points_per_obj;
        const unsigned v = (unsigned)(gp - obj * io.points_per_obj), nyz = (unsigned)(gm.n[1] * gm.n[2]);
        const unsigned i = v / nyz, jk = v - i * nyz, j = jk / (unsigned)gm.n[2], k = jk - j * (unsigned)gm.n[2];
        px = gm.lo[0] + gm.h[0] * (float)i; py = gm.lo[1] + gm.h[1] * (float)j; pz = gm.lo[2] + gm.h[2] * (float)k;
        dx = dy = dz = 0.f;
    } else {
        // the workgroup's brick (uniform: 512 points per brick); point l of the brick is (l >> 6, (l >> 3) & 7, l & 7) from its lowest corner.
        // A brick outside the object range or the lattice's brick range is computed on brick 0 of object 0 and stores nothing.
        const int* bk = gm.bricks + ((tile_wg * WGP) >> 9) * 4;
        const int nb0 = (gm.lat.n[0] + 7) >> 3, nb1 = (gm.lat.n[1] + 7) >> 3, nb2 = (gm.lat.n[2] + 7) >> 3;
        const bool ok = bk[0] >= 0 && bk[0] < gm.n_objects && bk[1] >= 0 && bk[1] < nb0 && bk[2] >= 0 && bk[2] < nb1 && bk[3] >= 0 && bk[3] < nb2;
        b_obj = ok ? bk[0] : 0;
        const unsigned l = (unsigned)(gp & 511);
        const unsigned i = 8u * (unsigned)(ok ? bk[1] : 0) + (l >> 6), j = 8u * (unsigned)(ok ? bk[2] : 0) + ((l >> 3) & 7u),
                       k = 8u * (unsigned)(ok ? bk[3] : 0) + (l & 7u);
        // mode 3's formula on the same (i, j, k): the same fp32 coordinates, so the same sigma bit for bit
        px = gm.lat.lo[0] + gm.lat.h[0] * (float)i; py = gm.lat.lo[1] + gm.lat.h[1] * (float)j; pz = gm.lat.lo[2] + gm.lat.h[2] * (float)k;
        dx = dy = dz = 0.f;
        b_keep = ok && i < (unsigned)gm.lat.n[0] && j < (unsigned)gm.lat.n[1] && k < (unsigned)gm.lat.n[2];
        b_dst = b_obj * ((long long)gm.lat.n[0] * gm.lat.n[1] * gm.lat.n[2]) + ((long long)i * gm.lat.n[1] + j) * gm.lat.n[2] + k;
    }
    const float* bias = lds + lo.bias;
    const float* heads = bias + L.n_mfma_layers * 256;       // sigma_w (256) | sigma_b | rgb2_w (384) | rgb2_b, as in the packed stream
    const float* zero = lds + lo.zero;
    // (mode 4: the brick's object for both; points_per_obj is the brick's 512 there)
    const float* lat_lane = io.latent + (MODE == 4 ? b_obj : gp / io.points_per_obj) * (long long)L.n_lat * 256;       // (!LATLDS: the lane's own object)
    const float* lat_wg = io.latent + (MODE == 4 ? b_obj : (tile_wg * WGP) / io.points_per_obj) * (long long)L.n_lat * 256;

    // ---- prologue: first weight chunk, biases + heads (+ latent rows) by LDS-DMA while the positional encodings are computed
    Ring16 ring;
    ring.cur = 0;
    Dma16 dm;
    dm.voff = lane * 16u + 4096u;
    dm.lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) float*)lds);
    dm.wave = __builtin_amdgcn_readfirstlane(wave);
    {
        const int sw = (n >> 1) & 7;
        ring.aoff[0] = n * KC + (((0 + g) ^ sw) << 2);
        ring.aoff[1] = n * KC + (((4 + g) ^ sw) << 2);
    }
    // the forward stream (snr_layout.h): enc_xyz 2 chunks, then 8 per 256-wide layer (9 for enc_viewdir: the direction chunk is its ninth),
    // rgb.0's 8 chunks of 128 rows.  A layer's FIRST consumed chunk is its chunk 0 -- enc_viewdir's is the direction chunk.
    constexpr long long C256 = 256 * KC;
    const int li_encshape = sb + 1, li_view = sb + 2, li_last = sb + tb + 2;
    const float* const stream = io.packed + L.fwd;
    auto layer_base = [&](int li) { return stream + 2 * C256 + (long long)(li - 1) * 8 * C256 + (li > li_view ? C256 : 0); };      // li = 1 .. li_last + 1
    auto layer_first = [&](int li) { return layer_base(li) + (li == li_view ? 8 * C256 : 0); };
    f32x4 xin[4], xd[2];
    {
        chunk_dma16<WAVES>(dm, stream, lds, lds, 256);
        for (int r = dm.wave; r < L.n_mfma_layers + 3; r += WAVES) row_dma16(dm, io.packed + L.bias + r * 256, lds + lo.bias + r * 256, lds);
        if (LATLDS)
            for (int r = dm.wave; r < L.n_lat; r += WAVES) row_dma16(dm, lat_wg + r * 256, lds + lo.lat + r * 256, lds);
        if (tid < 64) *reinterpret_cast<f32x4*>(lds + lo.zero + 4 * tid) = f32x4{0.f, 0.f, 0.f, 0.f};
        float* sc = lds + lo.scratch + wave * PE_WAVE16 + n * PE_ROW;
        // 30 (frequency, axis) pairs of the xyz encoding, 8 per lane group (the fourth takes 6); 12 of the direction encoding, 3 each
#pragma unroll 1
        for (int i = 0; i < 8; i += 2) {                   // two pairs per trip on packed arithmetic (pe_sincos2: half the VALU instructions)
            const int q = 8 * g + i;
            if (q < 3 * XYZ_FREQ) {
                f32x2 sn, cs;
                pe_sincos2(f32x2{ldexpf(pick3(px, py, pz, q % 3), q / 3), ldexpf(pick3(px, py, pz, (q + 1) % 3), (q + 1) / 3)}, &sn, &cs);
                sc[3 + q] = sn[0]; sc[3 + 3 * XYZ_FREQ + q] = cs[0];
                sc[4 + q] = sn[1]; sc[4 + 3 * XYZ_FREQ + q] = cs[1];
            }
        }
        if constexpr (!DENS) {
            const int q = 3 * g;
            f32x2 sn, cs;
            pe_sincos2(f32x2{ldexpf(pick3(dx, dy, dz, q % 3), q / 3), ldexpf(pick3(dx, dy, dz, (q + 1) % 3), (q + 1) / 3)}, &sn, &cs);
            sc[64 + 3 + q] = sn[0]; sc[64 + 3 + 3 * DIR_FREQ + q] = cs[0];
            sc[64 + 4 + q] = sn[1]; sc[64 + 4 + 3 * DIR_FREQ + q] = cs[1];
            float s1, c1;
            pe_sincos(ldexpf(pick3(dx, dy, dz, (q + 2) % 3), (q + 2) / 3), &s1, &c1);
            sc[64 + 5 + q] = s1; sc[64 + 5 + 3 * DIR_FREQ + q] = c1;
        }
        if (g == 0) {
            sc[0] = px; sc[1] = py; sc[2] = pz; sc[63] = 0.f;
            if constexpr (!DENS) {
                sc[64] = dx; sc[65] = dy; sc[66] = dz;
#pragma unroll
                for (int f = D_DIR; f < 32; ++f) sc[64 + f] = 0.f;
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        // B-operand registers: register r of input tile T <- feature 16 T + 4 g + r of the lane's point
#pragma unroll
        for (int T = 0; T < 4; ++T)
#pragma unroll
            for (int r = 0; r < 4; ++r) xin[T][r] = sc[16 * T + 4 * g + r];
#pragma unroll
        for (int T = 0; T < 2; ++T)
#pragma unroll
            for (int r = 0; r < 4; ++r) xd[T][r] = DENS ? 0.f : sc[64 + 16 * T + 4 * g + r];
        if (WAVES == 4) __syncthreads();      // the scratch lies over ring buffer 1: every wave has read its operands before any wave requests chunk 1
    }

    __builtin_amdgcn_s_setprio(0);
    SNR16_STAMP(1);
    // ---- enc_xyz: 64 -> 256 from explicit operand tiles (two chunks)
    f32x4 accP[16];
    f32x4 a0, a1;                    // the fragment pair in flight: the first of the chunk about to be consumed
    {
        f32x4 accC[16];
        acc_from_bias<16>(accC, bias, g);
#pragma unroll
        for (int ch = 0; ch < 2; ++ch) {
            chunk_dma16<WAVES>(dm, ch == 0 ? stream + C256 : layer_first(1), lds + (ring.cur ^ 1) * WBUF16, lds, 256);
            const float* wb = lds + ring.cur * WBUF16;
            first_pair(a0, a1, wb + ring.aoff[0]);
            tile_mma<16, false>(accC, accP, xin[2 * ch], wb + ring.aoff[0], a0, a1, wb + ring.aoff[1]);
            if (ch == 1) tile_mma<16, true>(accC, accP, xin[2 * ch + 1], wb + ring.aoff[1], a0, a1, nullptr);
            else tile_mma<16, false>(accC, accP, xin[2 * ch + 1], wb + ring.aoff[1], a0, a1, nullptr);
            ring_turn(ring);
        }
        first_pair(a0, a1, lds + ring.cur * WBUF16 + ring.aoff[0]);       // layer 1's: from here on the pair is carried (layer_from_acc)
    }

    SNR16_STAMP(2);
    // ---- the 256-wide middle layers (shape blocks, enc_shape, enc_viewdir, texture blocks): layer li consumes layer li - 1's sums
    uint32_t mw[4] = {0u, 0u, 0u, 0u};
    float o_sigma = 0.f;
    float pos_inf = __builtin_inff();
    asm volatile("" : "+v"(pos_inf));          // (opaque: a literal +inf in v_med3 would be rewritten as canonicalise + v_max, per value)
    auto epi_of = [&](int lp) {          // the epilogue applied to the OUTPUT of layer lp on its way into layer lp + 1
        const int la = latent_after(lp, sb, tb);
        Epi c;
        c.lo = (lp != li_encshape) ? 0.f : -__builtin_inff();
        c.zlds = (la >= 0) ? lds + lo.lat + la * 256 : zero;
        c.zglb = (la >= 0) ? lat_lane + la * 256 : nullptr;
        c.hi = pos_inf;
        return c;
    };
    auto after_layer_input = [&](int lp) {      // ReLU bits of layer lp, collected while it was consumed
        if (MASKS && lp != li_encshape && tile_live) store_masks16x4(io.masks + (tile32 * n_relu + relu_slot(lp, sb)) * 64, mw, wave, lane);
    };
    const int li_stop = DENS ? li_encshape : li_last;       // density only: the stream ends with enc_shape
    // enc_viewdir's direction chunk: once per workgroup when the workgroup is one ray of a fused render (uniform), else per point
    bool one_ray = false;
    if constexpr (MODE == 1) one_ray = gm.S == WGP;
#pragma unroll 1
    for (int li = 1; li <= li_stop; ++li) {
        const int lp = li - 1;
        const Epi c = epi_of(lp);
        if (!DENS && li == li_view) {
            SNR16_STAMP(3);
            // density head on enc_shape's finished sums (accP, no activation, no latent): softplus(w_sigma . y + b), src/model_supnerf.py:257.
            // One pass of 64 fma here instead of an fma + a head-weight fetch in EVERY layer's per-value epilogue: on this chip a VALU
            // instruction is not hidden by fp32 MFMAs, it competes with them for the same ALUs.  The lane groups hold a quarter of the features.
            float s = 0.f;
#pragma unroll
            for (int T = 0; T < 16; ++T) {
                const f32x4 ws = *reinterpret_cast<const f32x4*>(heads + 16 * T + 4 * g);
#pragma unroll
                for (int r = 0; r < 4; ++r) s = fmaf(ws[r], accP[T][r], s);
            }
            s += __shfl_xor(s, 16, 64);
            s += __shfl_xor(s, 32, 64);
            const float pre = s + heads[L.sigma_b - L.sigma_w];
            o_sigma = pre > 20.f ? pre : log1pf(expf(pre));
        }
        const bool end = DENS && li == li_stop;
        if constexpr (MODE == 1)
            layer_from_acc<16, WAVES, LATLDS, MASKS, true>(accP, ring, lds, bias + li * 256, c, g, dm, layer_base(li), li == li_view, xd, layer_first(li + 1),
                                                                 (li == li_last) ? 128 : 256, mw, a0, a1, one_ray, (one_ray && li + 1 == li_view) ? own_rows16<WAVES>(dm) : 0);
        else
        layer_from_acc<16, WAVES, LATLDS, MASKS>(accP, ring, lds, bias + li * 256, c, g, dm, layer_base(li), !DENS && li == li_view, xd,
                                                       end ? nullptr : layer_first(li + 1), end ? 0 : (li == li_last) ? 128 : 256, mw, a0, a1);
        after_layer_input(lp);
    }
    if constexpr (DENS) {
        // the density head above, the same instructions on the same sums.  (Kept as a copy: one helper for both places changes the register
        // allocation of the modes 0 / 1 instantiations, whose code this variant leaves as it was.)
        float s = 0.f;
#pragma unroll
        for (int T = 0; T < 16; ++T) {
            const f32x4 ws = *reinterpret_cast<const f32x4*>(heads + 16 * T + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; ++r) s = fmaf(ws[r], accP[T][r], s);
        }
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        const float pre = s + heads[L.sigma_b - L.sigma_w];
        o_sigma = pre > 20.f ? pre : log1pf(expf(pre));
        if constexpr (MODE == 4) {
            if (b_keep && g == 0) io.sigmas[b_dst] = o_sigma;
        } else {
            if (live && g == 0) io.sigmas[gp] = o_sigma;
        }
        return;
    }
    SNR16_STAMP(4);
    {   // rgb.0: 256 -> 128
        const Epi c = epi_of(li_last);
        layer_from_acc<8, WAVES, LATLDS, MASKS>(accP, ring, lds, bias + (li_last + 1) * 256, c, g, dm, layer_base(li_last + 1), false, xd, nullptr, 0, mw, a0, a1);
        after_layer_input(li_last);
    }

    SNR16_STAMP(5);
    __builtin_amdgcn_s_setprio(3);
    // ---- rgb.0's output (accP tiles 0..7): ReLU + bits, then rgb.2 (128 -> 3) on the VALU
    float o_r, o_g, o_b;
    {
        const float* w2 = heads + (L.rgb2_w - L.sigma_w);
        float pr = 0.f, pg = 0.f, pb = 0.f;
        uint32_t m16 = 0u, mr[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int T = 0; T < 8; ++T) {
            const f32x4 wr = *reinterpret_cast<const f32x4*>(w2 + 16 * T + 4 * g);
            const f32x4 wg = *reinterpret_cast<const f32x4*>(w2 + 128 + 16 * T + 4 * g);
            const f32x4 wb = *reinterpret_cast<const f32x4*>(w2 + 256 + 16 * T + 4 * g);
            f32x4 xv;
#pragma unroll
            for (int r = 3; r >= 0; --r) {
                float v = accP[T][r];
                m16 = __builtin_amdgcn_alignbit(m16, __float_as_uint(0.f - v), 31);
                v = fmaxf(v, 0.f);
                xv[r] = v;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) { pr = fmaf(wr[r], xv[r], pr); pg = fmaf(wg[r], xv[r], pg); pb = fmaf(wb[r], xv[r], pb); }
            if ((T & 3) == 3) { mr[T >> 2] = m16; m16 = 0u; }
        }
        if (MASKS && tile_live) store_masks16x4(io.masks + (tile32 * n_relu + (n_relu - 1)) * 64, mr, wave, lane);
        pr += __shfl_xor(pr, 16, 64); pr += __shfl_xor(pr, 32, 64);
        pg += __shfl_xor(pg, 16, 64); pg += __shfl_xor(pg, 32, 64);
        pb += __shfl_xor(pb, 16, 64); pb += __shfl_xor(pb, 32, 64);
        const float* b2 = heads + (L.rgb2_b - L.sigma_w);
        o_r = pr + b2[0]; o_g = pg + b2[1]; o_b = pb + b2[2];
    }

    SNR16_STAMP_HWID(6);
#ifndef SNR_STAMPS
    if (live && g == 0 && io.sigmas) io.sigmas[gp] = o_sigma;
#endif
    if (live && g == 0) {
        if (io.rgbs) { io.rgbs[gp * 3] = o_r; io.rgbs[gp * 3 + 1] = o_g; io.rgbs[gp * 3 + 2] = o_b; }
    }
    if constexpr (MODE == 1) {
        float* comp = lds + lo.comp;             // (WAVES = 4: over ring buffer 0 -- every wave is past the last chunk's barrier, reached with its last ring read returned: RingTurn)
        if (g == 0) {
            float* c = comp + (wave * 16 + n) * COMP_STRIDE;
            c[0] = o_sigma; c[1] = o_r; c[2] = o_g; c[3] = o_b; c[4] = zc;
        }
        __syncthreads();
        composite_rays_fwd<WGP, WAVES>(comp, gm.S, gm.flags & SNR_WHITE_BKGD, gm.n_rays, tile_wg, wave, lane, out_rgb, out_depth, out_acc);      // (the host guarantees WGP % S == 0)
    }
    SNR16_STAMP(7);
}

}  // namespace snr

using namespace snr;

// mode 0: explicit points; mode 1: fused render.  Two shapes of the same kernel:
//   WAVES = 4 -- 64 points per 256-thread workgroup, TWO workgroups per CU (each at most 80 KiB of LDS: its own two-buffer weight ring, the
//     decoder's biases / heads, latent rows).  The two waves of a SIMD then belong to DIFFERENT workgroups: they share no barrier, drift
//     out of phase, and whatever one is doing at a chunk rendezvous or a layer start the other's MFMAs fill the matrix pipe.  Costs twice the
//     L2 -> LDS weight traffic per point (8 B/clk/CU).  Taken whenever it fits: the ray (render mode) inside 64 points, LDS <= 80 KiB.
//   WAVES = 8 -- 128 points per 512-thread workgroup, one per CU; both waves of a SIMD run the same program between the same barriers.
// The workgroup's latent rows are staged in LDS when its points belong to ONE object and the table has at most LDS_LAT_ROWS rows.

template <int MODE, int WAVES, bool LATLDS, bool MASKS>
static int launch16(const DecoderIO& io, const Layout& L, const Lds16& lo, const float* xyz, const float* viewdir, const typename PointSrc<MODE>::T& g,
                    float* rgb, float* depth, float* acc, hipStream_t st) {
    auto kern = decoder_fwd16_kernel<MODE, WAVES, LATLDS, MASKS>;
    // Dynamic LDS beyond the default cap must be granted per kernel, and (if HIP scopes the attribute per device) per device: one bit per
    // device that has it.  nn.DataParallel enters here from one host thread per device.  Two threads may both grant it; that is harmless.
    static std::atomic<uint64_t> granted{0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return SNR_E_LAUNCH;
    const uint64_t bit = dev < 64 ? (uint64_t)1 << dev : 0;          // (devices past 64: granted on every launch)
    if (!(granted.load(std::memory_order_acquire) & bit)) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return SNR_E_LAUNCH;
        granted.fetch_or(bit, std::memory_order_release);
    }
    const unsigned grid = (unsigned)((io.n_points + WAVES * 16 - 1) / (WAVES * 16));
    kern<<<grid, WAVES * 64, (size_t)lo.total * 4, st>>>(io, L, lo, xyz, viewdir, g, rgb, depth, acc);
    return snr_check_launch_();
}

// The shape of a launch (see above), decided here for every launcher of this file: four waves whenever the map fits two workgroups per CU
// and a render's ray lies inside 64 points, else eight; the latent rows in LDS or not; the LDS map of that choice.
struct Shape16 { int waves; bool latlds; Lds16 lo; };
static Shape16 launch_shape16(int mode, const DecoderIO& io, const Layout& L, int S) {
    auto with = [&](int waves) {
        Shape16 s;
        s.waves = waves;
        s.latlds = (io.points_per_obj % (waves * 16)) == 0 && L.n_lat <= LDS_LAT_ROWS;
        s.lo = make_lds16(waves, L.n_mfma_layers, s.latlds ? L.n_lat : LDS_LAT_ROWS + 1);
        return s;
    };
    const Shape16 four = with(4);
    const bool fits = four.lo.total * 4 <= 80 * 1024 && (mode != MODE_RENDER || (S <= 64 && 64 % S == 0));
    return fits ? four : with(8);
}

// The one dispatch over (MODE, WAVES, LATLDS, MASKS): the launchers below name MODE and the shape's WAVES, this picks the instantiation for the
// shape's LATLDS and for MASKS (io.masks set; modes 3 and 4 save no ReLU bits and have no such kernels).  The order in which the instantiations
// are first named is the order of the kernels in the code object, and it is kept as it has been: that is why WAVES is chosen by the callers
// (modes 0 and 1 alternate inside each WAVES) and why the nesting of the two flags differs between the families.
template <int MODE, int WAVES>
static int launch16_flags(const Shape16& s, const DecoderIO& io, const Layout& L, const float* xyz, const float* viewdir, const typename PointSrc<MODE>::T& src,
                          float* rgb, float* depth, float* acc, hipStream_t st) {
    auto go = [&](auto latlds, auto masks) {
        return launch16<MODE, WAVES, decltype(latlds)::value, decltype(masks)::value>(io, L, s.lo, xyz, viewdir, src, rgb, depth, acc, st);
    };
    constexpr std::true_type Y{};
    constexpr std::false_type N{};
    const bool ll = s.latlds, mk = io.masks != nullptr;
    if constexpr (MODE == MODE_POINTS || MODE == MODE_RENDER) return ll ? (mk ? go(Y, Y) : go(Y, N)) : (mk ? go(N, Y) : go(N, N));
    else if constexpr (MODE == MODE_DENSITY) return mk ? (ll ? go(Y, Y) : go(N, Y)) : (ll ? go(Y, N) : go(N, N));
    else return ll ? go(Y, N) : go(N, N);
}

int snr_fp32_fwd16_launch_(int mode, const DecoderIO& io, const Layout& L, const float* xyz, const float* viewdir, const RayGeom& g, float* rgb,
                           float* depth, float* acc, void* stream_) {
    hipStream_t st = (hipStream_t)stream_;
    if (io.act) return SNR_E_UNSUPPORTED;          // (training dumps: snr_mlp.hip's kernel, whose dump stores are staged through LDS; this one has none)
    const Shape16 s = launch_shape16(mode, io, L, g.S);
    if (s.waves == 4) return mode == MODE_POINTS ? launch16_flags<MODE_POINTS, 4>(s, io, L, xyz, viewdir, g, rgb, depth, acc, st)
                                                 : launch16_flags<MODE_RENDER, 4>(s, io, L, xyz, viewdir, g, rgb, depth, acc, st);
    return mode == MODE_POINTS ? launch16_flags<MODE_POINTS, 8>(s, io, L, xyz, viewdir, g, rgb, depth, acc, st)
                               : launch16_flags<MODE_RENDER, 8>(s, io, L, xyz, viewdir, g, rgb, depth, acc, st);
}

// density only (modes 2, 3 and 4): the shapes and the latent staging of mode 0, no dumps.  Mode 2 saves the ReLU bits of enc_xyz and the shape
// layers when io.masks is set (the slots snr_decoder_fwd writes for them; the texture-branch slots are left as they are)
template <int MODE>
static int density_launch(const DecoderIO& io, const float* xyz, const typename PointSrc<MODE>::T& src, void* stream_) {
    const Layout L = make_layout(io.sb, io.tb);
    const Shape16 s = launch_shape16(MODE, io, L, 0);
    hipStream_t st = (hipStream_t)stream_;
    return s.waves == 4 ? launch16_flags<MODE, 4>(s, io, L, xyz, nullptr, src, nullptr, nullptr, nullptr, st)
                        : launch16_flags<MODE, 8>(s, io, L, xyz, nullptr, src, nullptr, nullptr, nullptr, st);
}

int snr_density_points_launch_(const DecoderIO& io, const float* xyz, void* stream_) { return density_launch<MODE_DENSITY>(io, xyz, RayGeom{}, stream_); }

// A launch is 4 threads per point and HIP caps a launch below 2^32 threads: at most 2^20 bricks (2^29 points) per launch, the list taken in pieces.
int snr_density_bricks_launch_(const DecoderIO& io_, const BrickSrc& src, long long n_bricks, void* stream_) {
    constexpr long long CHUNK = 1 << 20;
    for (long long off = 0; off < n_bricks; off += CHUNK) {
        const long long n = n_bricks - off < CHUNK ? n_bricks - off : CHUNK;
        DecoderIO io = io_;
        io.n_points = n * 512;
        const int rc = density_launch<MODE_BRICKS>(io, nullptr, BrickSrc{src.lat, src.bricks + off * 4, src.n_objects}, stream_);
        if (rc != SNR_OK) return rc;
    }
    return SNR_OK;
}

// (the launchers stay in this order: it is the order of the kernels in the code object)
int snr_density_lattice_launch_(const DecoderIO& io, const snr_lattice& lattice, void* stream_) { return density_launch<MODE_LATTICE>(io, nullptr, lattice, stream_); }
