// Backward of the scene composite (snr_aux.hip: scene_general_kernel) for gfx950: per pixel the depth merge of n = Nb*S samples, the
// analytic composite backward on the merged rows, and the way back through the merge to the samples.  HBM-bound: 20 B per sample in,
// 20 B per sample out.  The ranks over verified lists are the forward's own: snr_scene_merge.hpp.
#include "snr_device.hpp"
#include "snr_host.hpp"
#include "snr_scene_merge.hpp"

namespace snr {

constexpr int SCENE_BWD_MAX_N = 512;            // 8 objects x 64 samples; 7 n floats of LDS per wave, 56 KiB per workgroup there
constexpr uint32_t SCENE_NO_SURVIVOR = 0xffffu;

// One wave per pixel, grid-stride over pixels.  LDS per wave: the depth row in memory order | five sorted rows (sigma, r, g, b, z) that
// the composite backward reads and then overwrites, slot by slot, with its five gradients | one word per SAMPLE: its own slot pos_i
// (low half) and, for the survivor of a group of equal depths, the group's first slot lt_i (high half; SCENE_NO_SURVIVOR otherwise).
// The last pass gathers through that word: lane i writes sample i's five gradients, every output element once, no atomics.
template <int NCH>
__global__ void __launch_bounds__(256) scene_bwd_kernel(const float* __restrict__ sigmas, const float* __restrict__ rgbs, const float* __restrict__ zv,
                                                        long long n_pixels, int n, int run, int flags, const float* __restrict__ d_rgb,
                                                        const float* __restrict__ d_depth, const float* __restrict__ d_acc,
                                                        float* __restrict__ d_sigmas, float* __restrict__ d_rgbs, float* __restrict__ d_z) {
    extern __shared__ __attribute__((aligned(16))) float scene_bwd_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* zs = scene_bwd_lds + (size_t)wave * 7 * n;
    float* s_sig = zs + n; float* s_r = s_sig + n; float* s_g = s_r + n; float* s_b = s_g + n; float* s_z = s_b + n;
    uint32_t* slot = reinterpret_cast<uint32_t*>(s_z + n);
    const long long wave0 = (long long)blockIdx.x * 4 + wave;
    const long long n_waves = (long long)gridDim.x * 4;
    const bool white = flags & SNR_WHITE_BKGD;
    for (long long pix = wave0; pix < n_pixels; pix += n_waves) {
        const float* zrow = zv + pix * n;
        const float* srow = sigmas + pix * n;
        const float* crow = rgbs + pix * n * 3;
        for (int i = lane; i < n; i += 64) zs[i] = zrow[i];
        __builtin_amdgcn_wave_barrier();
        // sample i (depth zi, rank counts lt / eb / ea) -> the sorted rows, exactly as the forward places it
        auto place = [&](int i, float zi, int lt, int eb, int ea) {
            const int pos = lt + eb;
            s_z[pos] = zi;
            if (eb > 0) { s_sig[pos] = 0.f; s_r[pos] = 0.f; s_g[pos] = 0.f; s_b[pos] = 0.f; }
            if (ea == 0) { s_sig[lt] = srow[i]; s_r[lt] = crow[3 * i]; s_g[lt] = crow[3 * i + 1]; s_b[lt] = crow[3 * i + 2]; }
            slot[i] = (uint32_t)pos | ((ea == 0 ? (uint32_t)lt : SCENE_NO_SURVIVOR) << 16);
        };
        const bool merged = scene_lists_ascend(zs, n, run, lane);
        if (merged) {                                          // verified ascending lists: two binary searches per (sample, list)
            const int n_runs = n / run;
            for (int i = lane; i < n; i += 64) {
                const float zi = zs[i];
                const SceneRank k = scene_list_rank(zs, n_runs, run, i, zi);
                place(i, zi, k.lt, k.eb, k.ea);
            }
        }
        for (int base = 0; base < n && !merged; base += 256) {   // rank sort: up to four own samples per pass against broadcast reads
            float zi[4]; int lt[4], eb[4], ea[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) { const int i = base + 64 * c + lane; zi[c] = (i < n) ? zs[i] : 0.f; lt[c] = eb[c] = ea[c] = 0; }
            for (int j = 0; j < n; ++j) {
                const float zj = zs[j];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int i = base + 64 * c + lane;
                    lt[c] += (zj < zi[c]) ? 1 : 0;
                    eb[c] += (zj == zi[c] && j < i) ? 1 : 0;
                    ea[c] += (zj == zi[c] && j > i) ? 1 : 0;
                }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int i = base + 64 * c + lane;
                if (i < n) place(i, zi[c], lt[c], eb[c], ea[c]);
            }
        }
        __builtin_amdgcn_wave_barrier();
        const float gr = d_rgb[pix * 3], gg = d_rgb[pix * 3 + 1], gb = d_rgb[pix * 3 + 2];
        const float gd = d_depth ? d_depth[pix] : 0.f, ga = d_acc ? d_acc[pix] : 0.f;
        composite_ray_bwd<NCH>(n, lane, white, gr, gg, gb, gd, ga,
            [&](int k, float& sg, float& cr, float& cg, float& cb, float& z, float& zn) {
                sg = s_sig[k]; cr = s_r[k]; cg = s_g[k]; cb = s_b[k];
                z = s_z[k]; zn = (k < n - 1) ? s_z[k + 1] : 0.f;
            },
            [&](int k, float ds, float dcr, float dcg, float dcb, float dz) {
                __builtin_amdgcn_wave_barrier();               // every fetch of the wave is behind us: slot k now holds its gradients
                s_sig[k] = ds; s_r[k] = dcr; s_g[k] = dcg; s_b[k] = dcb; s_z[k] = dz;
            });
        __builtin_amdgcn_wave_barrier();
        float* ds_row = d_sigmas + pix * n;
        float* dc_row = d_rgbs + pix * n * 3;
        for (int i = lane; i < n; i += 64) {
            const uint32_t w = slot[i];
            const uint32_t pos = w & 0xffffu, lt = w >> 16;
            const bool survivor = lt != SCENE_NO_SURVIVOR;
            const uint32_t k = survivor ? lt : 0u;
            ds_row[i] = survivor ? s_sig[k] : 0.f;
            dc_row[3 * i] = survivor ? s_r[k] : 0.f; dc_row[3 * i + 1] = survivor ? s_g[k] : 0.f; dc_row[3 * i + 2] = survivor ? s_b[k] : 0.f;
            if (d_z) d_z[pix * n + i] = s_z[pos];
        }
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace snr

using namespace snr;

extern "C" {

int snr_scene_composite_bwd(const float* sigmas, const float* rgbs, const float* z_vals, int64_t n_pixels, int n_per_pixel, int run_length,
                            int flags, const float* d_rgb, const float* d_depth, const float* d_acc, float* d_sigmas, float* d_rgbs,
                            float* d_z, void* stream_) {
    if (n_pixels == 0) return SNR_OK;
    if (!sigmas || !rgbs || !z_vals || !d_rgb || !d_sigmas || !d_rgbs) return SNR_E_ARG;
    if (n_pixels < 0 || n_per_pixel < 1 || run_length < 0) return SNR_E_ARG;
    if (run_length > 0 && (n_per_pixel % run_length) != 0) return SNR_E_SHAPE;
    if (n_per_pixel > SCENE_BWD_MAX_N) return SNR_E_UNSUPPORTED;
    const size_t lds = (size_t)4 * 7 * n_per_pixel * sizeof(float);             /* <= 56 KiB: no attribute to raise */
    const long long blocks = (n_pixels + 3) / 4;
    const int grid = (int)(blocks > 8192 ? 8192 : blocks);
    hipStream_t st = (hipStream_t)stream_;
#define SNR_LAUNCH_SB(N) scene_bwd_kernel<N><<<grid, 256, lds, st>>>(sigmas, rgbs, z_vals, n_pixels, n_per_pixel, run_length, flags, d_rgb, d_depth, \
                                                                     d_acc, d_sigmas, d_rgbs, d_z)
    const int n = n_per_pixel;                                                   /* <= 256: the chunk counts snr_composite_bwd uses */
    if (n <= 64) SNR_LAUNCH_SB(1); else if (n <= 128) SNR_LAUNCH_SB(2); else if (n <= 192) SNR_LAUNCH_SB(3); else if (n <= 256) SNR_LAUNCH_SB(4);
    else if (n <= 384) SNR_LAUNCH_SB(6); else SNR_LAUNCH_SB(8);
#undef SNR_LAUNCH_SB
    return snr_check_launch_();
}

}  // extern "C"
