// The decoder's C ABI (include/supnerf_hip.h), host code only: the argument checks of its twelve entry points and the one place that decides
// which kernel family a call runs (the file map: DESIGN.md, section 4).  The kernels and their launch policy stay in the files this one calls
// through snr_host.hpp.  The order of the checks inside an entry point is part of its behaviour (tests/test_decoder_abi_cpu.py).
#include "snr_mlp_core.hpp"
#include "snr_grid.hpp"
#include "snr_host.hpp"

using namespace snr;

static DecoderIO decoder_io(const float* packed, const float* latent, int sb, int tb, long long n_points, long long points_per_obj, float* sigmas,
                            float* rgbs, void* relu_masks, float* activations) {
    return DecoderIO{packed, latent, sb, tb, n_points, points_per_obj, sigmas, rgbs, (uint4*)relu_masks, activations, false, nullptr};
}

// the fields every backward sets; the upstream gradients and the outputs are the entry point's own
static BwdIO bwd_io(const float* packed, const float* latent, int sb, int tb, long long n_points, long long points_per_obj, const void* relu_masks,
                    const float* sigmas) {
    BwdIO io{};
    io.packed = packed; io.latent = latent; io.sb = sb; io.tb = tb; io.n_points = n_points; io.points_per_obj = points_per_obj;
    io.masks = (const uint4*)relu_masks; io.sigmas = sigmas;
    return io;
}

// exact fp32: the two-waves-per-SIMD kernel (16x16x4, 16 points per wave); training dumps stay on the one-wave 32x32x2 kernel, whose
// LDS-staged dump stores write whole cache lines (13.9 against 14.2 ms per fp32 step)
static int decoder_forward(int mode, const DecoderIO& io, int precision, const float* xyz, const float* viewdir, const RayGeom& g, float* rgb,
                           float* depth, float* acc, void* stream_) {
    const Layout L = make_layout(io.sb, io.tb);
    if (precision == SNR_BF16X3) {
        if (!snr_bf16_supported_(io.sb, io.tb, io.points_per_obj)) return SNR_E_UNSUPPORTED;
        return snr_bf16_launch_fwd_(mode, io, L, xyz, viewdir, g, rgb, depth, acc, stream_);
    }
    if (precision != SNR_FP32) return SNR_E_ARG;
    if (io.act) return snr_fp32_train_fwd_launch_(io, L, xyz, viewdir, stream_);
    return snr_fp32_fwd16_launch_(mode, io, L, xyz, viewdir, g, rgb, depth, acc, stream_);
}

// The backward of every mode: choose the kernel, launch it and, where the latent gradient is wanted, sum the partial rows it wrote.
// Exact fp32 runs the two-waves-per-SIMD kernel where it applies (no training dumps, a ray inside 64 points, latent gradients only for objects
// of a multiple of 64 points -- always, for the density backward), else the one-wave 32x32x2 kernel.
// workspace = partial latent gradients [rows][n_lat][256] + the reduction tree's scratch; sized (snr_decoder_bwd_ws_bytes) for the smallest
// tile any kernel writes a row for: 32 points, a wave tile of the 32x32 and the split kernels; snr_mlp16_bwd.hip writes one row per 64-point
// workgroup.  A row must not straddle two objects.  The kernel that ran decides the points per row, and so where the scratch starts.
static int decoder_backward(int mode, BwdIO io, int precision, const float* xyz, const float* viewdir, const RayGeom& g, float* d_latent,
                            void* workspace, size_t ws_bytes, void* stream_) {
    const Layout L = make_layout(io.sb, io.tb);
    if (d_latent && L.n_lat > 0) {
        if (io.points_per_obj % (mode == MODE_DENSITY ? 64 : 32)) return SNR_E_UNSUPPORTED;
        if (!workspace || ws_bytes < snr_decoder_bwd_ws_bytes(io.n_points, io.points_per_obj, io.sb, io.tb)) return SNR_E_WORKSPACE;
        io.partial = (float*)workspace;
    }
    int rc, row;
    if (precision == SNR_BF16X3) {
        if (!snr_bf16_supported_(io.sb, io.tb, io.points_per_obj)) return SNR_E_UNSUPPORTED;
        row = 32;
        rc = snr_bf16_launch_bwd_(mode, io, L, xyz, viewdir, g, stream_);
    } else if (precision != SNR_FP32) {
        return SNR_E_ARG;
    } else if (snr_fp32_bwd16_supported_(mode, io, g)) {
        row = 64;
        rc = snr_fp32_bwd16_launch_(mode, io, L, xyz, viewdir, g, stream_);
    } else {
        row = 32;
        rc = snr_fp32_bwd32_launch_(mode, io, L, xyz, viewdir, g, stream_);
    }
    if (rc != SNR_OK || !io.partial) return rc;
    float* const scratch = io.partial + ((io.n_points + row - 1) / row) * (long long)L.n_lat * 256;
    return snr_launch_reduce_latent_(io.partial, scratch, io.points_per_obj / row, L.n_lat, io.n_points / io.points_per_obj, d_latent, stream_);
}

// snr_density_fwd, and with relu_masks snr_density_fwd_masks
static int density_points(const float* xyz, const float* latent, const float* packed, int64_t n_points, int64_t points_per_obj, int sb, int tb,
                          float* sigmas, void* relu_masks, void* stream_) {
    if (!xyz || !latent || !packed || !sigmas) return SNR_E_ARG;
    if (!blocks_ok(sb, tb) || n_points < 0) return SNR_E_ARG;
    if (!objects_ok(n_points, points_per_obj)) return SNR_E_SHAPE;
    if (n_points == 0) return SNR_OK;
    return snr_density_points_launch_(decoder_io(packed, latent, sb, tb, n_points, points_per_obj, sigmas, nullptr, relu_masks, nullptr), xyz, stream_);
}

extern "C" {

int snr_precision_supported(int precision, int sb, int tb, int64_t points_per_obj) {
    if (!blocks_ok(sb, tb)) return 0;
    if (precision == SNR_FP32) return 1;
    if (precision == SNR_BF16X3) return snr_bf16_supported_(sb, tb, points_per_obj);
    return 0;
}

int snr_decoder_fwd(const float* xyz, const float* viewdir, const float* latent, const float* packed, int64_t n_points,
                    int64_t points_per_obj, int sb, int tb, float* sigmas, float* rgbs, void* relu_masks, float* activations, int precision,
                    void* stream_) {
    if (!xyz || !viewdir || !latent || !packed) return SNR_E_ARG;
    if (activations && !relu_masks) return SNR_E_ARG;                         /* training dumps go with the ReLU bits */
    if (!blocks_ok(sb, tb) || n_points < 0) return SNR_E_ARG;
    if (!objects_ok(n_points, points_per_obj)) return SNR_E_SHAPE;
    if (n_points == 0) return SNR_OK;
    const DecoderIO io = decoder_io(packed, latent, sb, tb, n_points, points_per_obj, sigmas, rgbs, relu_masks, activations);
    return decoder_forward(MODE_POINTS, io, precision, xyz, viewdir, RayGeom{}, nullptr, nullptr, nullptr, stream_);
}

int snr_render_fwd(const snr_render_args* a, float* rgb, float* depth, float* acc_trans, float* sigmas, float* rgbs,
                   void* relu_masks, void* stream_) {
    RayGeom g;
    int rc = snr_fill_geom_(a, &g, 1);
    if (rc != SNR_OK) return rc;
    if (!rgb || !depth || !acc_trans) return SNR_E_ARG;
    if (a->n_samples > 128 || (128 % a->n_samples) != 0) return SNR_E_UNSUPPORTED;
    if (a->n_rays == 0) return SNR_OK;
    DecoderIO io = decoder_io(a->packed, a->latent, a->shape_blocks, a->texture_blocks, a->n_rays * a->n_samples, a->rays_per_obj * a->n_samples,
                              sigmas, rgbs, relu_masks, nullptr);
    io.latent_bias = a->latent_bias;
    return decoder_forward(MODE_RENDER, io, a->precision, nullptr, nullptr, g, rgb, depth, acc_trans, stream_);
}

int snr_density_fwd_masks(const float* xyz, const float* latent, const float* packed, int64_t n_points, int64_t points_per_obj, int sb, int tb,
                          float* sigmas, void* relu_masks, void* stream_) {
    if (!relu_masks) return SNR_E_ARG;
    return density_points(xyz, latent, packed, n_points, points_per_obj, sb, tb, sigmas, relu_masks, stream_);
}

int snr_density_fwd(const float* xyz, const float* latent, const float* packed, int64_t n_points, int64_t points_per_obj, int sb, int tb,
                    float* sigmas, void* stream_) {
    return density_points(xyz, latent, packed, n_points, points_per_obj, sb, tb, sigmas, nullptr, stream_);
}

// points_per_obj = one brick: the latent staging of a single-object workgroup applies (512 is a whole number of workgroups)
int snr_density_bricks(const snr_lattice* lattice, int64_t n_objects, const int32_t* bricks, int64_t n_bricks, const float* latent,
                       const float* packed, int sb, int tb, float* sigmas, void* stream_) {
    GridDims G;
    if (grid_check(lattice, n_objects, 1, G) != SNR_OK || !bricks || !latent || !packed || !sigmas) return SNR_E_ARG;
    if (!blocks_ok(sb, tb) || n_bricks < 0) return SNR_E_ARG;
    if (n_objects == 0 || n_bricks == 0) return SNR_OK;
    return snr_density_bricks_launch_(decoder_io(packed, latent, sb, tb, 0, 512, sigmas, nullptr, nullptr, nullptr),
                                      BrickSrc{*lattice, bricks, (long long)n_objects}, n_bricks, stream_);
}

int snr_density_grid(const snr_lattice* lattice, int64_t n_objects, const float* latent, const float* packed, int sb, int tb, float* sigmas,
                     void* stream_) {
    GridDims G;
    if (grid_check(lattice, n_objects, 1, G) != SNR_OK || !latent || !packed || !sigmas) return SNR_E_ARG;
    if (!blocks_ok(sb, tb)) return SNR_E_ARG;
    if (n_objects == 0) return SNR_OK;
    return snr_density_lattice_launch_(decoder_io(packed, latent, sb, tb, (long long)n_objects * G.nv, G.nv, sigmas, nullptr, nullptr, nullptr),
                                       *lattice, stream_);
}

size_t snr_decoder_bwd_ws_bytes(int64_t n_points, int64_t points_per_obj, int sb, int tb) {
    const int64_t tiles = (n_points + 31) / 32;
    const int64_t ppo = points_per_obj > 0 ? points_per_obj : n_points;
    const int64_t n_obj = ppo > 0 ? (n_points + ppo - 1) / ppo : 1;
    const int64_t tree = snr_reduce_scratch_floats_((ppo + 31) / 32, sb + tb, n_obj);
    return (size_t)((tiles * (int64_t)(sb + tb) * 256 + tree) * sizeof(float) + 256);
}

int snr_decoder_bwd(const float* xyz, const float* viewdir, const float* latent, const float* packed, const void* relu_masks,
                    const float* sigmas, const float* d_sigmas, const float* d_rgbs, int64_t n_points, int64_t points_per_obj, int sb,
                    int tb, float* d_latent, float* d_xyz, float* d_viewdir, float* layer_grads, void* workspace, size_t ws_bytes, int precision,
                    void* stream_) {
    if (n_points == 0) return SNR_OK;
    if (!xyz || !viewdir || !latent || !packed || !relu_masks || !sigmas) return SNR_E_ARG;
    if (!blocks_ok(sb, tb) || n_points < 0) return SNR_E_ARG;
    if (!objects_ok(n_points, points_per_obj)) return SNR_E_SHAPE;
    BwdIO io = bwd_io(packed, latent, sb, tb, n_points, points_per_obj, relu_masks, sigmas);
    io.d_sigmas = d_sigmas; io.d_rgbs = d_rgbs;
    io.d_xyz = d_xyz; io.d_dir = d_viewdir;
    io.gdump = layer_grads;
    return decoder_backward(MODE_POINTS, io, precision, xyz, viewdir, RayGeom{}, d_latent, workspace, ws_bytes, stream_);
}

// backward of snr_density_fwd: always the two-waves kernel, so its latent gradient needs whole 64-point workgroups per object
int snr_density_bwd(const float* xyz, const float* latent, const float* packed, const void* relu_masks, const float* sigmas,
                    const float* d_sigmas, int64_t n_points, int64_t points_per_obj, int sb, int tb, float* d_latent, float* d_xyz,
                    void* workspace, size_t ws_bytes, void* stream_) {
    if (!xyz || !latent || !packed || !relu_masks || !sigmas || !d_sigmas) return SNR_E_ARG;
    if (!blocks_ok(sb, tb) || n_points < 0) return SNR_E_ARG;
    if (!objects_ok(n_points, points_per_obj)) return SNR_E_SHAPE;
    if (n_points == 0) return SNR_OK;
    BwdIO io = bwd_io(packed, latent, sb, tb, n_points, points_per_obj, relu_masks, sigmas);
    io.d_sigmas = d_sigmas;
    io.d_xyz = d_xyz;
    return decoder_backward(MODE_DENSITY, io, SNR_FP32, xyz, nullptr, RayGeom{}, d_latent, workspace, ws_bytes, stream_);
}

size_t snr_render_bwd_ws_bytes(const snr_render_args* a) {
    if (!a) return 0;
    return snr_decoder_bwd_ws_bytes(a->n_rays * (int64_t)a->n_samples, a->rays_per_obj * (int64_t)a->n_samples, a->shape_blocks, a->texture_blocks);
}

int snr_render_bwd(const snr_render_args* a, const float* sigmas, const float* rgbs, const void* relu_masks, const float* d_rgb,
                   const float* d_depth, const float* d_acc, float* d_latent, float* d_rays_o, float* d_rays_d, float* d_t,
                   void* workspace, size_t ws_bytes, void* stream_) {
    RayGeom g;
    int rc = snr_fill_geom_(a, &g, 1);
    if (rc != SNR_OK) return rc;
    if (a->n_rays == 0) return SNR_OK;
    if (!sigmas || !rgbs || !relu_masks) return SNR_E_ARG;
    if (a->n_samples > 128 || (128 % a->n_samples) != 0) return SNR_E_UNSUPPORTED;
#ifndef SNR_STAMPS      /* the diagnostic build borrows d_t as its stamp buffer */
    if (d_t && a->z_mode != SNR_Z_PER_RAY) return SNR_E_UNSUPPORTED;
#endif
    BwdIO io = bwd_io(a->packed, a->latent, a->shape_blocks, a->texture_blocks, a->n_rays * a->n_samples, a->rays_per_obj * a->n_samples, relu_masks,
                      sigmas);
    io.rgbs = rgbs;
    io.d_rgb = d_rgb; io.d_depth = d_depth; io.d_acc = d_acc;
    io.d_rays_o = d_rays_o; io.d_rays_d = d_rays_d; io.d_t = d_t;
    return decoder_backward(MODE_RENDER, io, a->precision, nullptr, nullptr, g, d_latent, workspace, ws_bytes, stream_);
}

}  // extern "C"
