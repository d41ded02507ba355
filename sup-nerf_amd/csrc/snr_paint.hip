// Mesh painting: per-vertex colours of a packed triangle mesh from the photographs of its views, occlusion-aware.
//
// The rules are the header's (include/supnerf_hip.h, "Mesh painting"); tests/paint_restatement.py restates them in numpy.  In short: a
// vertex samples a view's image bilinearly at its projected position (pixel centres at integers), over those of its four taps that the
// rasteriser's depth buffer and the occupancy mask let through, renormalised by their weights; the view weighs cos^2 of the angle between
// the vertex normal and the direction to the camera; views are accumulated one launch each in ascending order; vertices no view saw are
// filled from their neighbours, one Jacobi round per launch.
//
// Gathers only: one thread per vertex reads its own taps (or its own neighbour list) and writes its own rows.  No LDS, no atomics, no
// launch reads what another thread of the same launch wrote: the same bits from run to run.
#include "snr_packed_mesh.hpp"
#include "snr_host.hpp"

namespace snr {

constexpr unsigned PAINT_MAX_BLOCKS = 2048;          // 8 workgroups of 256 threads on each of 256 CUs; more vertices take further passes

inline unsigned paint_blocks(long long n) {
    const long long b = (n + GRID_THREADS - 1) / GRID_THREADS;
    return (unsigned)(b < PAINT_MAX_BLOCKS ? b : PAINT_MAX_BLOCKS);
}

struct PaintView {               // one view, by value
    const float* image;          // (H, W, 3)
    const float* mask;           // (H, W) or null
    const float* depth;          // (H, W): the rasteriser's, 0 where empty
    int H, W;
    float centre[3];             // the camera centre in the frame of the stored vertices
    float tol, z_near;
    int k;                       // the view's index
};

struct PaintState {              // per vertex, updated in place
    float* sum_rgb;              // (sum V, 3)
    float* sum_w;                // (sum V)
    int* seen;                   // (sum V)
    float* best_w;               // (sum V)
    int* best;                   // (sum V)
    float* best_rgb;             // (sum V, 3)
};

// rule P1 along one axis of n pixels: the lower tap i0 and the weight t of the upper one; false = outside the footprint
__device__ __forceinline__ bool paint_axis(float u, int n, int& i0, float& t) {
    if (u < 0.0f || u > (float)(n - 1)) return false;
    if (n == 1) { i0 = 0; t = 0.0f; return true; }
    i0 = min((int)floorf(u), n - 2);
    t = u - (float)i0;
    return true;
}

// rule P3: the weight of the view at a vertex; 0 = the view does not see it
__device__ __forceinline__ float paint_facing(const float* __restrict__ x, const float* __restrict__ n, const float centre[3]) {
    const float d0 = centre[0] - x[0], d1 = centre[1] - x[1], d2 = centre[2] - x[2];
    const float dot = (n[0] * d0 + n[1] * d1) + n[2] * d2;
    const float nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    const float dd = (d0 * d0 + d1 * d1) + d2 * d2;
    const float den = nn * dd;
    if (!(dot > 0.0f) || !(den > 0.0f) || !(den < INFINITY)) return 0.0f;
    return (dot * dot) / den;
}

__global__ void __launch_bounds__(GRID_THREADS) paint_view_kernel(const float* __restrict__ screen, const float* __restrict__ verts,
                                                                  const float* __restrict__ normals, long long nV, PaintView p,
                                                                  PaintState st) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long g = grid_thread(); g < nV; g += stride) {
        const float u = screen[g * 3], v = screen[g * 3 + 1], z = screen[g * 3 + 2];
        // P1 (every comparison is false on a NaN)
        if (!(fabsf(u) < INFINITY) || !(fabsf(v) < INFINITY) || !(fabsf(z) < INFINITY) || z < p.z_near) continue;
        int x0, y0;
        float a, b;
        if (!paint_axis(u, p.W, x0, a) || !paint_axis(v, p.H, y0, b)) continue;
        // P3 (before the taps: a view that faces away reads no pixel)
        const float gw = normals ? paint_facing(verts + g * 3, normals + g * 3, p.centre) : 1.0f;
        if (!(gw > 0.0f)) continue;
        // P2
        const float wx[2] = {1.0f - a, a}, wy[2] = {1.0f - b, b};
        float s = 0.0f, c[3] = {0.0f, 0.0f, 0.0f};
        bool any = false;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int tx = t & 1, ty = t >> 1;
            if ((tx && p.W == 1) || (ty && p.H == 1)) continue;                      // the duplicate of a tap: not read, never valid
            const long long q = (long long)(y0 + ty) * p.W + (x0 + tx);
            const float dq = p.depth[q];
            if (!(dq > 0.0f) || (p.mask && !(p.mask[q] > 0.0f)) || !(z <= dq + p.tol)) continue;
            const float w = wx[tx] * wy[ty];
            const float* __restrict__ I = p.image + q * 3;
            if (!any) {
                s = w;
                for (int j = 0; j < 3; ++j) c[j] = w * I[j];
                any = true;
            } else {
                s = s + w;
                for (int j = 0; j < 3; ++j) c[j] = c[j] + w * I[j];
            }
        }
        if (!(s > 0.0f)) continue;
        for (int j = 0; j < 3; ++j) c[j] = c[j] / s;
        // P4
        for (int j = 0; j < 3; ++j) st.sum_rgb[g * 3 + j] = st.sum_rgb[g * 3 + j] + gw * c[j];
        st.sum_w[g] = st.sum_w[g] + gw;
        st.seen[g] = st.seen[g] + 1;
        if (gw > st.best_w[g]) {
            st.best_w[g] = gw;
            st.best[g] = p.k;
            for (int j = 0; j < 3; ++j) st.best_rgb[g * 3 + j] = c[j];
        }
    }
}

__global__ void __launch_bounds__(GRID_THREADS) paint_finish_kernel(const float* __restrict__ sum_rgb, const float* __restrict__ sum_w,
                                                                    const int* __restrict__ seen, const float* __restrict__ best_rgb,
                                                                    long long nV, int blend, float background, float* __restrict__ colors,
                                                                    int* __restrict__ filled) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long g = grid_thread(); g < nV; g += stride) {
        const bool hit = seen[g] > 0;
        for (int j = 0; j < 3; ++j)
            colors[g * 3 + j] = !hit ? background : blend ? best_rgb[g * 3 + j] : sum_rgb[g * 3 + j] / sum_w[g];
        filled[g] = hit ? 0 : -1;
    }
}

__global__ void __launch_bounds__(GRID_THREADS) paint_fill_kernel(const float* __restrict__ colors_in, const int* __restrict__ filled_in,
                                                                  const long long* __restrict__ nbr_start, const int* __restrict__ nbr,
                                                                  const long long* __restrict__ voff, long long B, long long nV,
                                                                  long long nE, int round, float* __restrict__ colors_out,
                                                                  int* __restrict__ filled_out) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long g = grid_thread(); g < nV; g += stride) {
        int f = filled_in[g];
        float c[3] = {colors_in[g * 3], colors_in[g * 3 + 1], colors_in[g * 3 + 2]};
        if (f < 0) {
            const MeshObject o = mesh_object(voff, mesh_entry_of(voff, B, g), nV);
            const SmoothRing r = smooth_ring(nbr_start, g, nE);
            double s[3] = {0.0, 0.0, 0.0};
            long long n = 0;
            for (long long e = r.begin; e < r.end; ++e) {                           // ascending: the order is the contract
                const int j = nbr[e];
                if (!mesh_index_ok(j, o.V)) continue;                               // (an entry out of range adds nothing)
                const long long gj = o.v0 + j;
                if (filled_in[gj] < 0) continue;
                for (int k = 0; k < 3; ++k) s[k] += (double)colors_in[gj * 3 + k];
                ++n;
            }
            if (n > 0) {
                for (int k = 0; k < 3; ++k) c[k] = (float)(s[k] / (double)n);
                f = round;
            }
        }
        for (int k = 0; k < 3; ++k) colors_out[g * 3 + k] = c[k];
        filled_out[g] = f;
    }
}

// do the n elements of `size` bytes at a and at b share a byte?
inline bool paint_overlap(const void* a, const void* b, int64_t n, size_t size) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, bytes = (uintptr_t)n * size;
    return x < y + bytes && y < x + bytes;
}

}  // namespace snr

using namespace snr;

extern "C" {

int snr_paint_view(const float* screen, const float* verts, const float* normals, int64_t n_verts, const float* image, const float* mask,
                   const float* depth, int height, int width, float centre_x, float centre_y, float centre_z, float tol, float z_near,
                   int view, float* sum_rgb, float* sum_w, int32_t* seen, float* best_w, int32_t* best, float* best_rgb, void* stream) {
    const int rc = packed_sizes(0, n_verts, 0);
    if (rc != SNR_OK) return rc;
    if (height < 0 || width < 0 || view < 0 || !(z_near > 0.0f) || !(tol >= 0.0f) || !(tol < INFINITY)) return SNR_E_ARG;
    if (height && width && (long long)height * width > 0x7fffffffll) return SNR_E_UNSUPPORTED;
    if (n_verts == 0 || height == 0 || width == 0) return SNR_OK;
    if (!screen || !image || !depth || !sum_rgb || !sum_w || !seen || !best_w || !best || !best_rgb || (normals && !verts)) return SNR_E_ARG;
    const PaintView p = {image, mask, depth, height, width, {centre_x, centre_y, centre_z}, tol, z_near, view};
    const PaintState st = {sum_rgb, sum_w, seen, best_w, best, best_rgb};
    paint_view_kernel<<<paint_blocks(n_verts), GRID_THREADS, 0, (hipStream_t)stream>>>(screen, verts, normals, n_verts, p, st);
    return snr_check_launch_();
}

int snr_paint_finish(const float* sum_rgb, const float* sum_w, const int32_t* seen, const float* best_rgb, int64_t n_verts, int blend,
                     float background, float* colors, int32_t* filled, void* stream) {
    const int rc = packed_sizes(0, n_verts, 0);
    if (rc != SNR_OK) return rc;
    if (blend != 0 && blend != 1) return SNR_E_ARG;
    if (n_verts == 0) return SNR_OK;
    if (!seen || !colors || !filled || (blend ? !best_rgb : (!sum_rgb || !sum_w))) return SNR_E_ARG;
    paint_finish_kernel<<<paint_blocks(n_verts), GRID_THREADS, 0, (hipStream_t)stream>>>(sum_rgb, sum_w, seen, best_rgb, n_verts, blend,
                                                                                         background, colors, filled);
    return snr_check_launch_();
}

int snr_paint_fill(const float* colors_in, const int32_t* filled_in, const int64_t* nbr_start, const int32_t* nbr, const int64_t* vert_offset,
                   int64_t n_objects, int64_t n_verts, int64_t n_edges, int round, float* colors_out, int32_t* filled_out, void* stream) {
    const int rc = packed_sizes(n_objects, n_verts, n_edges);
    if (rc != SNR_OK) return rc;
    if (round < 1) return SNR_E_ARG;
    if (n_verts == 0) return SNR_OK;
    if (n_objects == 0 || !colors_in || !filled_in || !nbr_start || !vert_offset || !colors_out || !filled_out || (n_edges && !nbr))
        return SNR_E_ARG;
    if (paint_overlap(colors_in, colors_out, n_verts * 3, sizeof(float)) || paint_overlap(filled_in, filled_out, n_verts, sizeof(int32_t)))
        return SNR_E_ARG;                                                           // a Jacobi round: the two buffers are apart
    paint_fill_kernel<<<paint_blocks(n_verts), GRID_THREADS, 0, (hipStream_t)stream>>>(
        colors_in, filled_in, (const long long*)nbr_start, nbr, (const long long*)vert_offset, n_objects, n_verts, n_edges, round, colors_out,
        filled_out);
    return snr_check_launch_();
}

}  // extern "C"
