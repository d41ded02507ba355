// Cross-view evaluation (OptimizerNuScenes.eval_cross_view, src/optimizer_nuscenes.py:1279-1410): the codes fitted to view ii of an instance
// are rendered from the camera of every view num and scored against THAT view's whitened crop and lidar returns.  The renders of P such
// (code row, target view) pairs ride in the fused launches as P "objects"; this unit reduces their outputs to one metric row per pair in
// one launch for gfx950.  The V views' targets, labels and measured depths are read THROUGH the pair's target view: nothing per-view is
// copied per pair.  HBM-bound and tiny (28 B per ray): one workgroup of 256 threads per pair, every thread owns the rays
// threadIdx.x + 256 k, deterministic wave -> workgroup reduction (snr_device.hpp's wave_sum, then the 4 wave partials through LDS, added
// in wave order), plain vector stores: no atomics, the same bits every run.
#include "snr_device.hpp"
#include "snr_host.hpp"

namespace snr {

// sum over the workgroup's 4 waves, result in every thread; `slot` = 4 floats of LDS; fixed association ((w0 + w1) + w2) + w3
__device__ __forceinline__ float cross_block_sum(float v, float* slot) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    const float s = ((slot[0] + slot[1]) + slot[2]) + slot[3];
    __syncthreads();
    return s;
}

// out[p] = {mse_fg, depth_err, sum |occ|} of pair p = (code row, target view); only the target view is read here
__global__ void __launch_bounds__(256) cross_metrics_kernel(const float* __restrict__ rgb, const float* __restrict__ depth_pred,
                                                            const float* __restrict__ tgt, const float* __restrict__ occ,
                                                            const float* __restrict__ lid_depth, const int32_t* __restrict__ lid_cnt,
                                                            const int32_t* __restrict__ pairs, long long n_views, long long n, long long n_l,
                                                            float* __restrict__ out) {
    __shared__ float red[4];
    const long long p = blockIdx.x;
    long long v = pairs[2 * p + 1];
    v = v < 0 ? 0 : (v >= n_views ? n_views - 1 : v);         // (the host refuses such a table; nothing is read out of bounds regardless)
    const float* __restrict__ rgb_p = rgb + p * n * 3;
    const float* __restrict__ tgt_v = tgt + v * n * 3;
    const float* __restrict__ occ_v = occ + v * n;
    float sa = 0.f, sq = 0.f;
    for (long long i = threadIdx.x; i < n; i += 256) {
        const float a = fabsf(occ_v[i]);
        const float dr = rgb_p[i * 3] - tgt_v[i * 3], dg = rgb_p[i * 3 + 1] - tgt_v[i * 3 + 1], db = rgb_p[i * 3 + 2] - tgt_v[i * 3 + 2];
        sa += a;
        sq += (dr * dr + dg * dg + db * db) * a;
    }
    float sd = 0.f;
    int cnt = 0;
    if (n_l > 0) {
        const int c = lid_cnt[v];
        cnt = c < 0 ? 0 : (c > n_l ? (int)n_l : c);
        for (long long k = threadIdx.x; k < cnt; k += 256) sd += fabsf(depth_pred[p * n_l + k] - lid_depth[v * n_l + k]);
    }
    const float sum_a = cross_block_sum(sa, red);
    const float sum_q = cross_block_sum(sq, red);
    const float sum_d = cross_block_sum(sd, red);
    if (threadIdx.x == 0) {
        out[p * 3 + 0] = sum_q / (sum_a + 1e-9f);             // :1359-1360
        out[p * 3 + 1] = sum_d / ((float)cnt + 1e-8f);        // :1378-1379
        out[p * 3 + 2] = sum_a;
    }
}

}  // namespace snr

using namespace snr;

extern "C" {

int snr_cross_metrics(const float* rgb, const float* depth_pred, const float* tgt, const float* occ, const float* lid_depth,
                      const int32_t* lid_cnt, const int32_t* pairs, const int32_t* pairs_host, int64_t n_pairs, int64_t n_views, int64_t n_codes,
                      int64_t n, int64_t n_l, float* out, void* stream) {
    if (n_pairs < 1 || n_views < 1 || n_codes < 1 || n < 1 || n_l < 0) return SNR_E_ARG;
    if (!rgb || !tgt || !occ || !pairs || !out) return SNR_E_ARG;
    if (n_l > 0 && (!depth_pred || !lid_depth || !lid_cnt)) return SNR_E_ARG;
    if (pairs_host)
        for (int64_t p = 0; p < n_pairs; ++p)
            if (pairs_host[2 * p] < 0 || pairs_host[2 * p] >= n_codes || pairs_host[2 * p + 1] < 0 || pairs_host[2 * p + 1] >= n_views) return SNR_E_ARG;
    if (n_pairs > 0x7fffffffLL || n_views > 0x7fffffffLL || n > (int64_t)1 << 40 || n_l > (int64_t)1 << 40) return SNR_E_UNSUPPORTED;
    cross_metrics_kernel<<<(unsigned)n_pairs, 256, 0, (hipStream_t)stream>>>(rgb, depth_pred, tgt, occ, lid_depth, lid_cnt, pairs, n_views, n, n_l, out);
    return snr_check_launch_();
}

}  // extern "C"
