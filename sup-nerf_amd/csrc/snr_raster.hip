// Mesh rasteriser: which face of a packed triangle mesh each pixel of a pinhole camera sees, how far away, and with which barycentric weights.
//
// The rules are the header's (include/supnerf_hip.h, "Mesh rasteriser"); tests/raster_restatement.py restates them in numpy.  In short:
// vertices are projected in fp32 and snapped to 1/256 pixel; orientation and coverage are exact int64 edge functions with a tie rule that
// gives a pixel centre on a shared edge to exactly one of the two faces; the depth is the perspective-correct camera z, three positive
// terms and one division; per pixel the smallest depth wins, ties to the smallest packed face index.
//
// Visibility is one 64-bit unsigned atomic min per covered pixel on the key (bits(depth) << 32) | face: integer, so the result does not
// depend on the order of the threads and has the same bits from run to run.  Nothing in the faces launch READS a key (the L2s of the eight
// XCDs are not coherent within a launch); the resolve launch after it reads them with plain loads.  No floating-point atomics, no LDS.
//
// One thread per face walks the face's box of candidate pixels: iso-surface triangles seen from a camera cover a few pixels or none.  A
// face whose box holds RASTER_BIG_BOX candidates or more would serialise one lane over all of them, so it is handed to its whole wave
// instead: a ballot finds such faces, each one's snapped vertices are broadcast by shuffles, and the 64 lanes stride its box.
#include "snr_packed_mesh.hpp"
#include "snr_host.hpp"

namespace snr {

#ifndef SNR_RASTER_BIG_BOX
#define SNR_RASTER_BIG_BOX 64        // (tools/raster_time.py times diagnostic builds with other values)
#endif
constexpr int RASTER_BIG_BOX = SNR_RASTER_BIG_BOX;           // candidate pixels from which a face's box is walked by the whole wave
constexpr unsigned long long RASTER_EMPTY = ~0ull;           // the key of a pixel no face covers
constexpr float RASTER_MAX_PIXEL = 4194304.0f;               // 2^22: a vertex this far from the origin of the image drops its face

struct RasterTri {               // a snapped face: everything coverage, depth and weights are computed from
    int xs[3], ys[3];            // screen position with 8 sub-pixel bits
    float iz[3];                 // 1 / z
};

// rule 2: the three projected vertices of a face, snapped; false = the face is dropped
__device__ __forceinline__ bool raster_snap(const float* __restrict__ screen, long long v0, const int idx[3], float z_near, RasterTri& t) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float* p = screen + (v0 + idx[k]) * 3;
        const float u = p[0], v = p[1], z = p[2];
        // (every comparison is false on a NaN)
        ok = ok && fabsf(u) < RASTER_MAX_PIXEL && fabsf(v) < RASTER_MAX_PIXEL && z >= z_near && z < INFINITY;
        t.xs[k] = (int)rintf(u * 256.0f);
        t.ys[k] = (int)rintf(v * 256.0f);
        t.iz[k] = 1.0f / z;
    }
    return ok;
}

// rule 3: A, exact (coordinates within +-2^30, differences within +-2^31, products below 2^62)
__device__ __forceinline__ long long raster_area(const RasterTri& t) {
    const long long x0 = t.xs[0], y0 = t.ys[0];
    return (t.xs[1] - x0) * (t.ys[2] - y0) - (t.xs[2] - x0) * (t.ys[1] - y0);
}

struct RasterEdges {
    long long dx[3], dy[3];      // s (b - a) of edge i, which runs from vertex a = i + 1 to b = i + 2 (mod 3)
    int tie[3];                  // 1 where the edge owns the pixel centres on it
    long long area;              // s A > 0
};
__device__ __forceinline__ void raster_edges(const RasterTri& t, long long A, RasterEdges& e) {
    const long long s = A > 0 ? 1 : -1;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int a = (i + 1) % 3, b = (i + 2) % 3;
        e.dx[i] = s * ((long long)t.xs[b] - t.xs[a]);
        e.dy[i] = s * ((long long)t.ys[b] - t.ys[a]);
        e.tie[i] = e.dy[i] > 0 || (e.dy[i] == 0 && e.dx[i] < 0);
    }
    e.area = s * A;
}

// rule 4: the three edge functions at the centre of pixel (px, py); true = covered
__device__ __forceinline__ bool raster_cover(const RasterTri& t, const RasterEdges& e, int px, int py, long long E[3]) {
    const long long X = 256ll * px, Y = 256ll * py;
    bool in = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int a = (i + 1) % 3;
        E[i] = e.dx[i] * (Y - t.ys[a]) - e.dy[i] * (X - t.xs[a]);
        in = in && E[i] + e.tie[i] > 0;
    }
    return in;
}

// rule 5: q, the denominator of the depth and of the weights
__device__ __forceinline__ float raster_q(const RasterTri& t, const long long E[3]) {
    return ((float)E[0] * t.iz[0] + (float)E[1] * t.iz[1]) + (float)E[2] * t.iz[2];
}

struct RasterBox {
    int x0, x1, y0, y1;          // candidate pixels, both ends included
};
// the pixels whose centres lie in the snapped bounding box and in the image; returns how many
__device__ __forceinline__ int raster_box(const RasterTri& t, int W, int H, RasterBox& b) {
    const int xmin = min(t.xs[0], min(t.xs[1], t.xs[2])), xmax = max(t.xs[0], max(t.xs[1], t.xs[2]));
    const int ymin = min(t.ys[0], min(t.ys[1], t.ys[2])), ymax = max(t.ys[0], max(t.ys[1], t.ys[2]));
    b.x0 = max((xmin + 255) >> 8, 0);                  // (an arithmetic shift: the floor, below zero too)
    b.x1 = min(xmax >> 8, W - 1);
    b.y0 = max((ymin + 255) >> 8, 0);
    b.y1 = min(ymax >> 8, H - 1);
    if (b.x1 < b.x0 || b.y1 < b.y0) return 0;
    return (b.x1 - b.x0 + 1) * (b.y1 - b.y0 + 1);      // (at most H W < 2^31)
}

// rules 4 - 6 at one pixel of the face's image
__device__ __forceinline__ void raster_draw(const RasterTri& t, const RasterEdges& e, int px, int py, unsigned face,
                                            unsigned long long* image_keys, int W) {
    long long E[3];
    if (!raster_cover(t, e, px, py, E)) return;
    const float depth = (float)e.area / raster_q(t, E);
    atomicMin(image_keys + (long long)py * W + px, ((unsigned long long)__float_as_uint(depth) << 32) | face);
}

__global__ void raster_project_kernel(const float* __restrict__ verts, const long long* __restrict__ voff, long long B, long long nV,
                                      const float* __restrict__ obj_to_cam, float fx, float fy, float cx, float cy,
                                      float* __restrict__ screen) {
    const long long g = grid_thread();
    if (g >= nV) return;
    const float* M = obj_to_cam + mesh_entry_of(voff, B, g) * 12;
    const float x = verts[g * 3], y = verts[g * 3 + 1], z = verts[g * 3 + 2];
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = ((M[k * 4] * x + M[k * 4 + 1] * y) + M[k * 4 + 2] * z) + M[k * 4 + 3];
    screen[g * 3] = fx * (c[0] / c[2]) + cx;
    screen[g * 3 + 1] = fy * (c[1] / c[2]) + cy;
    screen[g * 3 + 2] = c[2];
}

__global__ void __launch_bounds__(GRID_THREADS) raster_faces_kernel(const float* __restrict__ screen, const int* __restrict__ faces,
                                                                    const long long* __restrict__ voff, const long long* __restrict__ foff,
                                                                    const int* __restrict__ image_of, const int* __restrict__ cull_sign,
                                                                    long long B, long long nV, long long nF, long long n_images, int H, int W,
                                                                    float z_near, unsigned long long* keys) {
    const long long f = grid_thread();
    const int lane = threadIdx.x & 63;
    RasterTri t = {};
    RasterBox box = {};
    long long A = 0, image = 0;
    int count = 0;                                       // candidate pixels; 0 for a dropped face and past the end of the list
    if (f < nF) {
        const MeshFace m = mesh_face(faces, voff, foff, B, nV, f);
        image = image_of[m.b];
        bool ok = m.ok && image >= 0 && image < n_images;
        if (ok) ok = raster_snap(screen, m.v0, m.idx, z_near, t);
        if (ok) {
            A = raster_area(t);
            const int front = cull_sign ? cull_sign[m.b] : 0;
            ok = A != 0 && !((A > 0 && front > 0) || (A < 0 && front < 0));
        }
        if (ok) count = raster_box(t, W, H, box);
    }
    const long long image_px = (long long)H * W;
    if (count > 0 && count < RASTER_BIG_BOX) {           // a thread per face
        RasterEdges e;
        raster_edges(t, A, e);
        unsigned long long* image_keys = keys + image * image_px;
        for (int py = box.y0; py <= box.y1; ++py)
            for (int px = box.x0; px <= box.x1; ++px) raster_draw(t, e, px, py, (unsigned)f, image_keys, W);
    }
    unsigned long long left = __ballot(count >= RASTER_BIG_BOX);
    while (left) {                                       // a wave per face (wave-uniform: every lane takes part in the shuffles)
        const int leader = __ffsll((long long)left) - 1;
        left &= left - 1;
        RasterTri bt;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            bt.xs[k] = __shfl(t.xs[k], leader);
            bt.ys[k] = __shfl(t.ys[k], leader);
            bt.iz[k] = __shfl(t.iz[k], leader);
        }
        const unsigned face = (unsigned)(f - lane + leader);
        unsigned long long* image_keys = keys + __shfl(image, leader) * image_px;
        RasterEdges e;
        RasterBox bb;
        raster_edges(bt, raster_area(bt), e);
        const int n = raster_box(bt, W, H, bb), bw = bb.x1 - bb.x0 + 1;
        const int step_x = 64 % bw, step_y = 64 / bw;                                // (wave-uniform: the only divisions of the walk)
        int px = bb.x0 + lane % bw, py = bb.y0 + lane / bw;
        for (int i = lane; i < n; i += 64) {                                         // candidate i = (py - y0) bw + (px - x0)
            raster_draw(bt, e, px, py, face, image_keys, W);
            px += step_x;
            py += step_y;
            if (px > bb.x1) { px -= bw; ++py; }
        }
    }
}

// a later launch: the keys are final and read with plain loads
__global__ void raster_resolve_kernel(const unsigned long long* __restrict__ keys, const float* __restrict__ screen,
                                      const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
                                      long long B, long long nV, long long nF, long long n_pixels, int H, int W, int* __restrict__ face_out,
                                      float* __restrict__ depth_out, float* __restrict__ weights) {
    const long long p = grid_thread();
    if (p >= n_pixels) return;
    const unsigned long long key = keys[p];
    const long long f = (long long)(key & 0xffffffffull);
    int face = -1;
    float depth = 0.0f, w[3] = {0.0f, 0.0f, 0.0f};
    MeshFace m;
    if (key != RASTER_EMPTY && f < nF && (m = mesh_face(faces, voff, foff, B, nV, f)).ok) {
        const long long rest = p % ((long long)H * W);
        RasterTri t;
        RasterEdges e;
        long long E[3];
        raster_snap(screen, m.v0, m.idx, 0.0f, t);
        raster_edges(t, raster_area(t), e);
        raster_cover(t, e, (int)(rest % W), (int)(rest / W), E);
        const float q = raster_q(t, E);
#pragma unroll
        for (int i = 0; i < 3; ++i) w[i] = ((float)E[i] * t.iz[i]) / q;
        depth = __uint_as_float((unsigned)(key >> 32));
        face = (int)f;
    }
    face_out[p] = face;
    depth_out[p] = depth;
#pragma unroll
    for (int i = 0; i < 3; ++i) weights[p * 3 + i] = w[i];
}

// one thread per pixel and channel
__global__ void raster_interpolate_kernel(const int* __restrict__ face, const float* __restrict__ weights, const int* __restrict__ faces,
                                          const long long* __restrict__ voff, const long long* __restrict__ foff, long long B, long long nV,
                                          long long nF, const float* __restrict__ attributes, int C, long long n_values, float background,
                                          float* __restrict__ out) {
    const long long g = grid_thread();
    if (g >= n_values) return;
    const long long p = g / C;
    const int c = (int)(g - p * C);
    const long long f = face[p];
    float v = background;
    MeshFace m;
    if (f >= 0 && f < nF && (m = mesh_face(faces, voff, foff, B, nV, f)).ok) {
        const float* w = weights + p * 3;
        v = (w[0] * attributes[(m.v0 + m.idx[0]) * C + c] + w[1] * attributes[(m.v0 + m.idx[1]) * C + c]) +
            w[2] * attributes[(m.v0 + m.idx[2]) * C + c];
    }
    out[g] = v;
}

// the sizes every entry point of the rasteriser shares; n_pixels = n_images H W
static int raster_sizes(int64_t n_objects, int64_t n_verts, int64_t n_faces, int64_t n_images, int H, int W, long long& n_pixels) {
    if (n_objects < 0 || n_verts < 0 || n_faces < 0 || n_images < 0 || H < 0 || W < 0) return SNR_E_ARG;
    n_pixels = 0;
    if (n_images && H && W) {
        if (n_images > 0x7fffffffll || (long long)H * W > 0x7fffffffll / n_images) return SNR_E_UNSUPPORTED;
        n_pixels = n_images * H * W;
    }
    if (n_objects > 0x7fffffffll || n_verts > (1ll << 38) || n_faces > 0x7fffffffll) return SNR_E_UNSUPPORTED;
    return SNR_OK;
}

}  // namespace snr

using namespace snr;

extern "C" {

int snr_raster_project(const float* verts, const int64_t* vert_offset, int64_t n_objects, int64_t n_verts, const float* obj_to_cam, float fx,
                       float fy, float cx, float cy, float* screen, void* stream) {
    long long n_pixels;
    const int rc = raster_sizes(n_objects, n_verts, 0, 0, 0, 0, n_pixels);
    if (rc != SNR_OK) return rc;
    if (n_verts == 0) return SNR_OK;
    if (n_objects == 0 || !verts || !vert_offset || !obj_to_cam || !screen) return SNR_E_ARG;
    raster_project_kernel<<<grid_blocks(n_verts), GRID_THREADS, 0, (hipStream_t)stream>>>(verts, (const long long*)vert_offset, n_objects,
                                                                                          n_verts, obj_to_cam, fx, fy, cx, cy, screen);
    return snr_check_launch_();
}

int snr_raster_faces(const float* screen, const int32_t* faces, const int64_t* vert_offset, const int64_t* face_offset,
                     const int32_t* image_of_object, const int32_t* cull_sign, int64_t n_objects, int64_t n_verts, int64_t n_faces,
                     int64_t n_images, int height, int width, float z_near, uint64_t* keys, void* stream) {
    long long n_pixels;
    const int rc = raster_sizes(n_objects, n_verts, n_faces, n_images, height, width, n_pixels);
    if (rc != SNR_OK) return rc;
    if (!(z_near > 0.0f)) return SNR_E_ARG;
    if (n_faces == 0 || n_pixels == 0) return SNR_OK;
    if (n_objects == 0 || !screen || !faces || !vert_offset || !face_offset || !image_of_object || !keys) return SNR_E_ARG;
    raster_faces_kernel<<<grid_blocks(n_faces), GRID_THREADS, 0, (hipStream_t)stream>>>(
        screen, faces, (const long long*)vert_offset, (const long long*)face_offset, image_of_object, cull_sign, n_objects, n_verts, n_faces,
        n_images, height, width, z_near, (unsigned long long*)keys);
    return snr_check_launch_();
}

int snr_raster_resolve(const uint64_t* keys, const float* screen, const int32_t* faces, const int64_t* vert_offset, const int64_t* face_offset,
                       int64_t n_objects, int64_t n_verts, int64_t n_faces, int64_t n_images, int height, int width, int32_t* face,
                       float* depth, float* weights, void* stream) {
    long long n_pixels;
    const int rc = raster_sizes(n_objects, n_verts, n_faces, n_images, height, width, n_pixels);
    if (rc != SNR_OK) return rc;
    if (n_pixels == 0) return SNR_OK;
    if (!keys || !face || !depth || !weights || (n_faces && (n_objects == 0 || !screen || !faces || !vert_offset || !face_offset)))
        return SNR_E_ARG;
    raster_resolve_kernel<<<grid_blocks(n_pixels), GRID_THREADS, 0, (hipStream_t)stream>>>(
        (const unsigned long long*)keys, screen, faces, (const long long*)vert_offset, (const long long*)face_offset, n_objects, n_verts,
        n_faces, n_pixels, height, width, face, depth, weights);
    return snr_check_launch_();
}

int snr_raster_interpolate(const int32_t* face, const float* weights, const int32_t* faces, const int64_t* vert_offset,
                           const int64_t* face_offset, int64_t n_objects, int64_t n_verts, int64_t n_faces, const float* attributes,
                           int n_channels, int64_t n_pixels, float background, float* out, void* stream) {
    long long none;
    const int rc = raster_sizes(n_objects, n_verts, n_faces, 0, 0, 0, none);
    if (rc != SNR_OK) return rc;
    if (n_pixels < 0 || n_channels < 1 || n_channels > PACKED_MAX_CHANNELS) return SNR_E_ARG;
    if (n_pixels > 0x7fffffffll) return SNR_E_UNSUPPORTED;
    if (n_pixels == 0) return SNR_OK;
    if (!face || !weights || !out || (n_faces && (n_objects == 0 || !faces || !vert_offset || !face_offset || !attributes))) return SNR_E_ARG;
    const long long n_values = n_pixels * n_channels;
    raster_interpolate_kernel<<<grid_blocks(n_values), GRID_THREADS, 0, (hipStream_t)stream>>>(
        face, weights, faces, (const long long*)vert_offset, (const long long*)face_offset, n_objects, n_verts, n_faces, attributes, n_channels,
        n_values, background, out);
    return snr_check_launch_();
}

}  // extern "C"
