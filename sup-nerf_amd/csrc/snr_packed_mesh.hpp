// What the packed-mesh kernels (snr_mesh.hip, snr_simplify.hip, snr_smooth.hip, snr_raster.hip, snr_paint.hip) share, stated once: the offset
// search, the face loader, the neighbour-list reader, the size limits and the fixed-order float64 segmented sum.  The specification is include/supnerf_hip.h ("Mesh components": the packed form;
// "Fixed-order segmented sums": the order, which tests/test_segment_sum_gpu.py holds the kernels to).  Functions only (see snr_grid.hpp).
#pragma once
#include "snr_grid.hpp"

namespace snr {

// ---- packed meshes: verts (sum V, 3) and object-local faces (sum F, 3) of several objects, object after
// object, with (n + 1) ascending int64 offsets that say where each object's vertices / faces start
// entry b of the (n + 1) ascending offsets `off` that holds item i: the largest b < n with off[b] <= i (empty entries are skipped)
__device__ __forceinline__ long long mesh_entry_of(const long long* __restrict__ off, long long n, long long i) {
    long long lo = 0, hi = n;
    while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

struct MeshObject {
    long long v0;                // where the object's vertices start
    long long V;                 // how many it has; 0 when the offsets are not usable
};
__device__ __forceinline__ MeshObject mesh_object(const long long* __restrict__ voff, long long b, long long nV) {
    MeshObject o;
    o.v0 = voff[b];
    o.V = voff[b + 1] - o.v0;
    if (o.v0 < 0 || o.V < 0 || o.V > 0x7fffffffll || o.v0 + o.V > nV) o.V = 0;
    return o;
}
__device__ __forceinline__ bool mesh_index_ok(int i, long long V) { return i >= 0 && (long long)i < V; }

// packed face f (0 <= f < sum F): its object, that object's vertices and its three indices, range-checked here, before anything is read
// with them.  What a bad face costs is the caller's: a flag, a skipped term or a dropped face.
struct MeshFace {
    long long b, v0, V;          // object, where its vertices start and how many it has (MeshObject)
    int idx[3];                  // local to the object
    bool ok;                     // all three in [0, V)
};
__device__ __forceinline__ MeshFace mesh_face(const int* __restrict__ faces, const long long* __restrict__ voff,
                                              const long long* __restrict__ foff, long long B, long long nV, long long f) {
    MeshFace m;
    m.b = mesh_entry_of(foff, B, f);
    const MeshObject o = mesh_object(voff, m.b, nV);
    m.v0 = o.v0; m.V = o.V;
    m.idx[0] = faces[f * 3]; m.idx[1] = faces[f * 3 + 1]; m.idx[2] = faces[f * 3 + 2];
    m.ok = mesh_index_ok(m.idx[0], o.V) && mesh_index_ok(m.idx[1], o.V) && mesh_index_ok(m.idx[2], o.V);
    return m;
}

// ---- the vertex adjacency of "Mesh smoothing" (a CSR over all vertices of the call), read by snr_smooth.hip and snr_paint.hip
// the neighbour list of packed vertex g, range-checked: entries [begin, end) of nbr; empty where nbr_start is not usable
struct SmoothRing {
    long long begin, end;
    __device__ __forceinline__ long long degree() const { return end - begin; }
};
__device__ __forceinline__ SmoothRing smooth_ring(const long long* __restrict__ nbr_start, long long g, long long nE) {
    SmoothRing r;
    r.begin = nbr_start[g];
    r.end = nbr_start[g + 1];
    if (r.begin < 0 || r.end < r.begin || r.end > nE) r.begin = r.end = 0;
    return r;
}

constexpr long long PACKED_MAX_ITEMS = 1ll << 38;    // items (vertices, faces, corners, ...) of one launch: blocks of 256 threads fit a 1-D grid
constexpr int PACKED_MAX_CHANNELS = 16;              // per-vertex attribute channels (rasteriser and simplification)

// the sizes every entry point over a packed mesh checks first: the object count and two item counts
inline int packed_sizes(int64_t n_objects, int64_t a, int64_t b) {
    if (n_objects < 0 || a < 0 || b < 0) return SNR_E_ARG;
    if (n_objects > 0x7fffffffll || a > PACKED_MAX_ITEMS || b > PACKED_MAX_ITEMS) return SNR_E_UNSUPPORTED;
    return SNR_OK;
}

// ---- the fixed-order float64 segmented sum (include/supnerf_hip.h, "Fixed-order segmented sums").  A list sorted by segment; slab s of
// segment c is the entries [seg_start[c] + 4096 j, + 4096), j = s - slab_off[c].  A workgroup per slab: thread t adds the slab's entries
// t, t + 256, ... in that order (the caller's loop, from 0.0), then block_tree.  A wave per segment: wave_sum.
constexpr int SEGMENT_SLAB = 4096;                   // sorted entries one workgroup sums (snr_segment_slab_bound, snr_mesh.hip, counts them)

struct SegmentSlab {
    long long c, begin, end;          // segment, entries [begin, end) of the sorted list; c < 0: no such slab.  Uniform over the block
};
__device__ __forceinline__ SegmentSlab segment_slab(const long long* __restrict__ seg_start, const long long* __restrict__ slab_off,
                                                    long long nC, long long n_items) {
    SegmentSlab r;
    const long long s = blockIdx.x;
    r.c = -1; r.begin = r.end = 0;
    if (s >= slab_off[nC]) return r;                                         // (the grid is an upper bound of the slab count)
    r.c = mesh_entry_of(slab_off, nC, s);
    r.begin = seg_start[r.c] + (s - slab_off[r.c]) * SEGMENT_SLAB;
    r.end = r.begin + SEGMENT_SLAB;
    if (r.end > seg_start[r.c + 1]) r.end = seg_start[r.c + 1];
    if (r.begin < 0) r.begin = 0;
    if (r.end > n_items) r.end = n_items;
    return r;
}

// a binary tree over the 256 threads in LDS, k = 128, 64, ..., 1: s[t] += s[t + k]; thread 0 writes the N sums.  s_sum: N * GRID_THREADS
template <int N>
__device__ __forceinline__ void block_tree(double (&acc)[N], double* __restrict__ s_sum, double* __restrict__ out) {
    const int t = threadIdx.x;
    for (int j = 0; j < N; ++j) s_sum[j * GRID_THREADS + t] = acc[j];
    for (int k = GRID_THREADS / 2; k; k >>= 1) {
        __syncthreads();
        if (t < k)
            for (int j = 0; j < N; ++j) s_sum[j * GRID_THREADS + t] += s_sum[j * GRID_THREADS + t + k];
    }
    if (t == 0)
        for (int j = 0; j < N; ++j) out[j] = s_sum[j * GRID_THREADS];
}

// per segment, lane l of a wave adds the slab sums l, l + 64, ... in that order (from 0.0), then a butterfly over the 64 lanes (xor 32,
// 16, ..., 1): every lane ends with the N sums.  Slab s has its sums at partial[s * stride .. + N)
template <int N>
__device__ __forceinline__ void wave_sum(const double* __restrict__ partial, long long stride, long long begin, long long end,
                                         long long n_slabs, int lane, double (&acc)[N]) {
    if (begin < 0) begin = 0;
    if (end > n_slabs) end = n_slabs;
    for (int j = 0; j < N; ++j) acc[j] = 0.0;
    for (long long s = begin + lane; s < end; s += 64)
        for (int j = 0; j < N; ++j) acc[j] += partial[s * stride + j];
    for (int k = 32; k; k >>= 1)
        for (int j = 0; j < N; ++j) acc[j] += __shfl_xor(acc[j], k);
}

}  // namespace snr
