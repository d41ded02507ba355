// Several views of one instance share one shape code and one texture code (src/optimizer_nuscenes.py:796-1277,
// optimize_objs_multi_anns / optimize_objs_multi_anns_w_pose).  The render, loss and pose launches take V "objects"; the codes have
// I <= V rows.  The two small pieces that tie them, as single launches for gfx950:
//   * view_pixels:   the iteration's random pixels of every view's NATIVE-resolution roi (render_rays, src/utils.py:380-432): pixel
//                    direction table, target colours and occupancy labels of the picked pixels, ragged crops, rectangular (V,n) output;
//                    a pick outside the crop is a padding ray with occupancy 0, which the loss tail weighs with exactly 0;
//   * instance_rows: row v of the (V,C) table is the row of v's instance; backward sums an instance's views in ascending order with
//                    plain fp32 adds, one thread per (instance, column): no atomics, the same bits every run.
// Both are memory-bound and tiny: a thread per output element, coalesced along the fastest axis.
#include "snr_host.hpp"
#include <hip/hip_runtime.h>

namespace snr {

__global__ void __launch_bounds__(256) view_pixels_kernel(const float* __restrict__ img, const float* __restrict__ occ,
                                                          const int64_t* __restrict__ crop_offset, const int32_t* __restrict__ roi,
                                                          const float* __restrict__ Kvec, const int32_t* __restrict__ picks, long long n_views,
                                                          long long n, float* __restrict__ cam_dirs, float* __restrict__ rgb_tgt,
                                                          float* __restrict__ occ_out) {
    const long long total = n_views * n;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const long long v = e / n;
        const int x0 = roi[4 * v], y0 = roi[4 * v + 1];
        const long long w = (long long)roi[4 * v + 2] - x0, h = (long long)roi[4 * v + 3] - y0;
        const long long base = crop_offset[v], room = crop_offset[v + 1] - base;
        const long long id = picks[e];
        float dx = 0.f, dy = 0.f, r = 0.f, g = 0.f, b = 0.f, o = 0.f;
        // a pixel of the crop: inside h*w AND inside the view's slice of the concatenated buffers (nothing is read otherwise)
        if (w > 0 && h > 0 && id >= 0 && id < w * h && id < room && base >= 0) {
            const float fx = Kvec[4 * v], fy = Kvec[4 * v + 1], cx = Kvec[4 * v + 2], cy = Kvec[4 * v + 3];
            const float x = (float)(x0 + (int)(id % w)), y = (float)(y0 + (int)(id / w));       // integers: exact in fp32
            dx = (x - cx) / fx;
            dy = (y - cy) / fy;
            const long long p = base + id;
            r = img[3 * p]; g = img[3 * p + 1]; b = img[3 * p + 2];
            o = occ[p];
        }
        cam_dirs[3 * e] = dx; cam_dirs[3 * e + 1] = dy; cam_dirs[3 * e + 2] = 1.f;
        rgb_tgt[3 * e] = r; rgb_tgt[3 * e + 1] = g; rgb_tgt[3 * e + 2] = b;
        occ_out[e] = o;
    }
}

// block (v, column chunk): the instance of view v is the last i with view_offset[i] <= v (uniform over the block)
__global__ void __launch_bounds__(256) instance_rows_fwd_kernel(const float* __restrict__ src, const int64_t* __restrict__ view_offset,
                                                                long long n_instances, long long n_cols, float* __restrict__ dst) {
    const long long v = blockIdx.x;
    long long lo = 0, hi = n_instances - 1;
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (view_offset[mid] <= v) lo = mid; else hi = mid - 1;
    }
    const long long c = (long long)blockIdx.y * blockDim.x + threadIdx.x;
    if (c < n_cols) dst[v * n_cols + c] = src[lo * n_cols + c];
}

// thread (i, c): d_src[i,c] = ((g[v0,c] + g[v0+1,c]) + ...) over the instance's views, ascending, starting from the first term
__global__ void __launch_bounds__(256) instance_rows_bwd_kernel(const float* __restrict__ d_dst, const int64_t* __restrict__ view_offset,
                                                                long long n_views, long long n_cols, float* __restrict__ d_src) {
    const long long i = blockIdx.x;
    const long long c = (long long)blockIdx.y * blockDim.x + threadIdx.x;
    if (c >= n_cols) return;
    long long v0 = view_offset[i], v1 = view_offset[i + 1];
    if (v0 < 0) v0 = 0;
    if (v1 > n_views) v1 = n_views;
    float acc = 0.f;
    if (v0 < v1) {
        acc = d_dst[v0 * n_cols + c];
        for (long long v = v0 + 1; v < v1; ++v) acc = acc + d_dst[v * n_cols + c];
    }
    d_src[i * n_cols + c] = acc;
}

// the (I+1) offsets as the host knows them: 0 = first, strictly ascending (no instance without a view), last = V
static int offsets_ok(const int64_t* off, int64_t n_instances, int64_t n_views) {
    if (off[0] != 0 || off[n_instances] != n_views) return 0;
    for (int64_t i = 0; i < n_instances; ++i)
        if (off[i + 1] <= off[i]) return 0;
    return 1;
}

static int rows_args(const int64_t* view_offset, const int64_t* view_offset_host, int64_t n_instances, int64_t n_views, int64_t n_cols) {
    if (n_instances < 1 || n_views < n_instances || n_cols < 1) return SNR_E_ARG;       // (V < I: some instance has no view)
    if (view_offset_host && !offsets_ok(view_offset_host, n_instances, n_views)) return SNR_E_ARG;
    if (!view_offset) return SNR_E_ARG;
    if (n_views > 0x7fffffffLL || n_instances > 0x7fffffffLL || (n_cols + 255) / 256 > 65535) return SNR_E_UNSUPPORTED;
    return SNR_OK;
}

}  // namespace snr

using namespace snr;

extern "C" {

int snr_view_pixels(const float* img, const float* occ, const int64_t* crop_offset, const int32_t* roi, const float* Kvec, const int32_t* picks,
                    int64_t n_views, int64_t n, float* cam_dirs, float* rgb_tgt, float* occ_out, void* stream) {
    if (n_views < 0 || n < 0) return SNR_E_ARG;
    if (n_views == 0 || n == 0) return SNR_OK;
    if (!img || !occ || !crop_offset || !roi || !Kvec || !picks || !cam_dirs || !rgb_tgt || !occ_out) return SNR_E_ARG;
    if (n_views > (int64_t)1 << 40 || n > (int64_t)1 << 40 || n_views * n > (int64_t)1 << 40) return SNR_E_UNSUPPORTED;
    long long blocks = (n_views * n + 255) / 256;
    if (blocks > 1024) blocks = 1024;                    // (beyond 262144 rays the threads stride)
    view_pixels_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(img, occ, crop_offset, roi, Kvec, picks, n_views, n, cam_dirs, rgb_tgt,
                                                                          occ_out);
    return snr_check_launch_();
}

int snr_instance_rows_fwd(const float* src, const int64_t* view_offset, const int64_t* view_offset_host, int64_t n_instances, int64_t n_views,
                          int64_t n_cols, float* dst, void* stream) {
    const int rc = rows_args(view_offset, view_offset_host, n_instances, n_views, n_cols);
    if (rc != SNR_OK) return rc;
    if (!src || !dst) return SNR_E_ARG;
    instance_rows_fwd_kernel<<<dim3((unsigned)n_views, (unsigned)((n_cols + 255) / 256)), 256, 0, (hipStream_t)stream>>>(src, view_offset, n_instances,
                                                                                                                       n_cols, dst);
    return snr_check_launch_();
}

int snr_instance_rows_bwd(const float* d_dst, const int64_t* view_offset, const int64_t* view_offset_host, int64_t n_instances, int64_t n_views,
                          int64_t n_cols, float* d_src, void* stream) {
    const int rc = rows_args(view_offset, view_offset_host, n_instances, n_views, n_cols);
    if (rc != SNR_OK) return rc;
    if (!d_dst || !d_src) return SNR_E_ARG;
    instance_rows_bwd_kernel<<<dim3((unsigned)n_instances, (unsigned)((n_cols + 255) / 256)), 256, 0, (hipStream_t)stream>>>(d_dst, view_offset, n_views,
                                                                                                                           n_cols, d_src);
    return snr_check_launch_();
}

}  // extern "C"
