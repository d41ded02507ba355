// Ray-cast surfaces: the per-ray passes around the density-only decoder that find the first point where sigma rises through a level.
//
// The rule is the header's (include/supnerf_hip.h, "Ray-cast surfaces"); tests/ray_restatement.py restates it in numpy, and the output of
// these kernels is bit-identical to it.  In short, for an interval [ta, tb] marched with S samples:
//   step = (tb - ta) / (S - 1),  t_k = ta + step k (k < S - 1),  t_{S-1} = tb exactly,  p_k = o + t_k d (one multiply, one add per axis);
//   a sample is inside iff sigma_k >= level; the first crossing is the smallest k with sigma_k outside and sigma_{k+1} inside;
//   its bracket (t_k, t_{k+1}, sigma_k, sigma_{k+1}) is marched again by the same kernels (refinement), and finally
//   t = ta + (level - va) / (vb - va) * (tb - ta),  x = o + t d.
// The decoder runs between these passes (snr_density_fwd on the point list); nothing here reads the weights.
//
// Three memory-bound passes of at most 16 bytes per sample next to a decoder launch of 557 kFLOP per sample.  The point list: a thread per
// sample (consecutive threads write consecutive points).  The hit points: a thread per ray.  The crossing search: a thread per ray for
// S < 32 (a refinement march; the row is a cache line or less), a wave per ray from S = 32 on (64 consecutive samples per load, the first
// crossing of a chunk by ballot).  No LDS, no atomics: the result is the same bit for bit from run to run.
#include "snr_device.hpp"
#include "snr_grid.hpp"
#include "snr_host.hpp"

namespace snr {

constexpr int RAY_WAVE_FROM = 32;            // samples per ray from which the crossing search takes a wave per ray
constexpr long long RAY_MAX_THREADS = 1ll << 31;

// depth of sample k of the march of [ta, tb] with S samples: the last sample is tb itself
__device__ __forceinline__ float ray_sample_t(float ta, float tb, int S, int k) {
    const float step = (tb - ta) / (float)(S - 1);
    return k == S - 1 ? tb : ta + step * (float)k;
}

__device__ __forceinline__ bool ray_inside(float sigma, float level) { return sigma >= level; }      // a NaN is outside

__global__ void ray_march_points_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d, const float* __restrict__ ta,
                                        const float* __restrict__ tb, long long total, int S, float* __restrict__ xyz) {
    const long long gid = grid_thread();
    if (gid >= total) return;
    const long long r = gid / S;
    const int k = (int)(gid - r * S);
    const float t = ray_sample_t(ta[r], tb[r], S, k);
    for (int a = 0; a < 3; ++a) xyz[gid * 3 + a] = rays_o[r * 3 + a] + t * rays_d[r * 3 + a];
}

// What one ray does with the outcome of its search.  k < 0: no crossing.  First march: the state is decided here, and a ray without a
// bracket (state 0 / 2) gets the dummy interval [ta, ta] with va = vb = 0.  Refinement: only state-1 rays are searched at all, and one
// whose march shows no crossing (possible only if sigma is not the decoder's at these points) keeps the bracket it had.
__device__ __forceinline__ void ray_store_bracket(long long r, int k, int S, bool first, bool starts_inside, float s_k, float s_k1,
                                                  float* __restrict__ ta, float* __restrict__ tb, float* __restrict__ va,
                                                  float* __restrict__ vb, unsigned char* __restrict__ state) {
    const float a = ta[r], b = tb[r];
    if (first) {
        const unsigned char st = starts_inside ? 2 : (k >= 0 ? 1 : 0);
        state[r] = st;
        if (st != 1) {
            tb[r] = a;
            va[r] = 0.f;
            vb[r] = 0.f;
            return;
        }
    } else if (k < 0) {
        return;
    }
    ta[r] = ray_sample_t(a, b, S, k);
    tb[r] = ray_sample_t(a, b, S, k + 1);
    va[r] = s_k;
    vb[r] = s_k1;
}

__global__ void ray_first_crossing_thread_kernel(const float* __restrict__ sigmas, long long n_rays, int S, float level, int first,
                                                 float* __restrict__ ta, float* __restrict__ tb, float* __restrict__ va,
                                                 float* __restrict__ vb, unsigned char* __restrict__ state) {
    const long long r = grid_thread();
    if (r >= n_rays) return;
    if (!first && state[r] != 1) return;
    const float* s = sigmas + r * S;
    float cur = s[0];
    const bool starts_inside = ray_inside(cur, level);
    int found = -1;
    float s_k = 0.f, s_k1 = 0.f;
    if (!(first && starts_inside)) {
        for (int k = 0; k < S - 1; ++k) {
            const float nxt = s[k + 1];
            if (!ray_inside(cur, level) && ray_inside(nxt, level)) {
                found = k; s_k = cur; s_k1 = nxt;
                break;
            }
            cur = nxt;
        }
    }
    ray_store_bracket(r, found, S, first != 0, starts_inside, s_k, s_k1, ta, tb, va, vb, state);
}

// a wave per ray: lane l of chunk c looks at the pair (64 c + l, 64 c + l + 1); the lowest set bit of the ballot is the chunk's first crossing
__global__ void ray_first_crossing_wave_kernel(const float* __restrict__ sigmas, long long n_rays, int S, float level, int first,
                                               float* __restrict__ ta, float* __restrict__ tb, float* __restrict__ va,
                                               float* __restrict__ vb, unsigned char* __restrict__ state) {
    const long long gid = grid_thread();
    const long long r = gid >> 6;
    const int lane = (int)(gid & 63);
    if (r >= n_rays) return;                                  // (whole waves: 256 threads per block, 64 per ray)
    if (!first && state[r] != 1) return;
    const float* s = sigmas + r * S;
    const bool starts_inside = ray_inside(s[0], level);
    int found = -1;
    if (!(first && starts_inside)) {
        for (int base = 0; base < S - 1; base += 64) {
            const int k = base + lane;
            const bool cross = k < S - 1 && !ray_inside(s[k], level) && ray_inside(s[k + 1], level);
            const unsigned long long m = __ballot(cross);
            if (m) {
                found = base + (int)__ffsll((long long)m) - 1;
                break;
            }
        }
    }
    if (lane != 0) return;
    const float s_k = found >= 0 ? s[found] : 0.f, s_k1 = found >= 0 ? s[found + 1] : 0.f;
    ray_store_bracket(r, found, S, first != 0, starts_inside, s_k, s_k1, ta, tb, va, vb, state);
}

__global__ void ray_hit_points_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d, const float* __restrict__ ta,
                                      const float* __restrict__ tb, const float* __restrict__ va, const float* __restrict__ vb,
                                      const unsigned char* __restrict__ state, long long n_rays, float level, float* __restrict__ depth,
                                      float* __restrict__ width, float* __restrict__ xyz) {
    const long long r = grid_thread();
    if (r >= n_rays) return;
    const unsigned char st = state[r];
    float t = 0.f, w = 0.f;
    if (st == 1) {
        const float a = ta[r], b = tb[r], fa = va[r], fb = vb[r];
        w = b - a;
        t = a + (level - fa) / (fb - fa) * w;
    } else if (st == 2) {
        t = ta[r];                                            // the dummy interval [near, near]
    }
    depth[r] = t;
    width[r] = w;
    for (int a = 0; a < 3; ++a) xyz[r * 3 + a] = rays_o[r * 3 + a] + t * rays_d[r * 3 + a];
}

static int ray_check(int64_t n_rays, int n_samples, long long threads_per_ray) {
    if (n_rays < 0) return SNR_E_ARG;
    if (n_samples < 2) return SNR_E_ARG;
    if (n_rays > RAY_MAX_THREADS / threads_per_ray) return SNR_E_UNSUPPORTED;
    return SNR_OK;
}

}  // namespace snr

using namespace snr;

extern "C" {

int snr_ray_march_points(const float* rays_o, const float* rays_d, const float* ta, const float* tb, int64_t n_rays, int n_samples,
                         float* xyz, void* stream) {
    const int rc = ray_check(n_rays, n_samples, n_samples);
    if (rc != SNR_OK) return rc;
    if (n_rays == 0) return SNR_OK;
    if (!rays_o || !rays_d || !ta || !tb || !xyz) return SNR_E_ARG;
    const long long total = (long long)n_rays * n_samples;
    ray_march_points_kernel<<<grid_blocks(total), GRID_THREADS, 0, (hipStream_t)stream>>>(rays_o, rays_d, ta, tb, total, n_samples, xyz);
    return snr_check_launch_();
}

int snr_ray_first_crossing(const float* sigmas, int64_t n_rays, int n_samples, float level, int first, float* ta, float* tb, float* va,
                           float* vb, uint8_t* state, void* stream) {
    const bool wave = n_samples >= RAY_WAVE_FROM;
    const int rc = ray_check(n_rays, n_samples, wave ? 64 : 1);
    if (rc != SNR_OK) return rc;
    if (first != 0 && first != 1) return SNR_E_ARG;
    if (n_rays == 0) return SNR_OK;
    if (!sigmas || !ta || !tb || !va || !vb || !state) return SNR_E_ARG;
    if (wave)
        ray_first_crossing_wave_kernel<<<grid_blocks((long long)n_rays * 64), GRID_THREADS, 0, (hipStream_t)stream>>>(
            sigmas, n_rays, n_samples, level, first, ta, tb, va, vb, state);
    else
        ray_first_crossing_thread_kernel<<<grid_blocks(n_rays), GRID_THREADS, 0, (hipStream_t)stream>>>(
            sigmas, n_rays, n_samples, level, first, ta, tb, va, vb, state);
    return snr_check_launch_();
}

int snr_ray_hit_points(const float* rays_o, const float* rays_d, const float* ta, const float* tb, const float* va, const float* vb,
                       const uint8_t* state, int64_t n_rays, float level, float* depth, float* width, float* xyz, void* stream) {
    const int rc = ray_check(n_rays, 2, 1);
    if (rc != SNR_OK) return rc;
    if (n_rays == 0) return SNR_OK;
    if (!rays_o || !rays_d || !ta || !tb || !va || !vb || !state || !depth || !width || !xyz) return SNR_E_ARG;
    ray_hit_points_kernel<<<grid_blocks(n_rays), GRID_THREADS, 0, (hipStream_t)stream>>>(rays_o, rays_d, ta, tb, va, vb, state, n_rays, level,
                                                                                         depth, width, xyz);
    return snr_check_launch_();
}

}  // extern "C"
