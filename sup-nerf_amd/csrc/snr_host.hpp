// Host side of libsupnerf_hip.so, stated once: every function that one translation unit defines and another calls, and the argument checks
// the entry points share.  Kernel arguments are forward-declared (snr_device.hpp, snr_mlp_core.hpp): a unit that only passes them on needs
// no kernel header.
#pragma once
#include "snr_layout.h"
#include "../../include/supnerf_hip.h"

namespace snr {
struct RayGeom; struct DecoderIO; struct BwdIO;

// Where a launch's points come from: modes 0 and 2 read xyz, mode 1 makes them on rays (RayGeom), mode 3 on a lattice, mode 4 in listed
// bricks of a lattice.  Modes 2 to 4 are density only (no view direction, nothing after the density head).
enum : int { MODE_POINTS = 0, MODE_RENDER = 1, MODE_DENSITY = 2, MODE_LATTICE = 3, MODE_BRICKS = 4 };
struct BrickSrc {
    snr_lattice lat;
    const int* bricks;           // (n_bricks, 4) int32: object, I, J, K -- brick (I, J, K) owns the points [8I, 8I+8) x [8J, 8J+8) x [8K, 8K+8)
    long long n_objects;
};

inline bool blocks_ok(int sb, int tb) { return sb >= 0 && tb >= 0 && sb <= MAX_BLOCKS && tb <= MAX_BLOCKS; }
// whole objects: SNR_E_SHAPE where this fails
inline bool objects_ok(long long n_points, long long points_per_obj) { return points_per_obj >= 1 && (n_points % points_per_obj) == 0; }
}  // namespace snr

// ---- snr_aux.hip
// validate snr_render_args and decode it into the by-value kernel argument
int snr_fill_geom_(const snr_render_args* a, snr::RayGeom* g, int need_model);
// SNR_OK, or SNR_E_LAUNCH with the HIP error kept for snr_last_hip_error
int snr_check_launch_(void);
// scratch needed behind the [obj][tiles][cols] partials for the reduction tree (floats), and the tree itself
long long snr_reduce_scratch_floats_(long long tiles_per_obj, int n_lat, long long n_obj);
int snr_launch_reduce_latent_(const float* partial, float* scratch, long long tiles_per_obj, int n_lat, long long n_obj, float* d_latent, void* stream);
// ---- snr_bf16.hip: the split ("bf16x3") arithmetic, modes 0 and 1; partial rows of 32 points
int snr_bf16_supported_(int sb, int tb, long long points_per_obj);
int snr_bf16_pack_(const float* const* t /* snr_pack_weights' tensor list */, int sb, int tb, float* packed, void* stream_);
int snr_bf16_launch_fwd_(int mode, const snr::DecoderIO& io, const snr::Layout& L, const float* xyz, const float* viewdir, const snr::RayGeom& g, float* rgb,
                         float* depth, float* acc, void* stream_);
int snr_bf16_launch_bwd_(int mode, const snr::BwdIO& io, const snr::Layout& L, const float* xyz, const float* viewdir, const snr::RayGeom& g, void* stream_);
// ---- snr_mlp.hip: the exact-fp32 training forward (mode 0 with activation dumps), one wave per SIMD
int snr_fp32_train_fwd_launch_(const snr::DecoderIO& io, const snr::Layout& L, const float* xyz, const float* viewdir, void* stream_);
// ---- snr_mlp16.hip: every other exact-fp32 forward (modes 0 and 1, no dumps), two waves per SIMD; the density launch per point source
int snr_fp32_fwd16_launch_(int mode, const snr::DecoderIO& io, const snr::Layout& L, const float* xyz, const float* viewdir, const snr::RayGeom& g, float* rgb,
                           float* depth, float* acc, void* stream_);
int snr_density_points_launch_(const snr::DecoderIO& io, const float* xyz, void* stream_);
int snr_density_lattice_launch_(const snr::DecoderIO& io, const snr_lattice& lattice, void* stream_);
// (io.n_points is set there, per piece of the list: 512 per brick)
int snr_density_bricks_launch_(const snr::DecoderIO& io, const snr::BrickSrc& src, long long n_bricks, void* stream_);
// ---- snr_mlp_bwd.hip: the exact-fp32 backward with one wave per SIMD (modes 0 and 1), partial rows of 32 points
int snr_fp32_bwd32_launch_(int mode, const snr::BwdIO& io, const snr::Layout& L, const float* xyz, const float* viewdir, const snr::RayGeom& g, void* stream_);
// ---- snr_mlp16_bwd.hip: the exact-fp32 backward with two waves per SIMD (modes 0 to 2) where it applies, partial rows of 64 points
int snr_fp32_bwd16_supported_(int mode, const snr::BwdIO& io, const snr::RayGeom& g);
int snr_fp32_bwd16_launch_(int mode, const snr::BwdIO& io, const snr::Layout& L, const float* xyz, const float* viewdir, const snr::RayGeom& g, void* stream_);
