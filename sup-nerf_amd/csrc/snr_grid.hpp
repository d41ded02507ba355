// The lattice and Kuhn-edge rules of the geometry kernels (snr_iso.hip, snr_iso_grad.hip, snr_band.hip; the density entry points of
// snr_decoder.hip use the host part), stated once; the packed-mesh kernels (snr_packed_mesh.hpp) take the launch shape from here.  The
// specification is include/supnerf_hip.h ("Geometry", "Narrow band", "Iso-surface backward").  Functions only, no __constant__ object: a
// table here would be copied into every code object that includes the header.
//
//   * a grid of n0 x n1 x n2 points per object, x-major (z fastest): point (i, j, k) has the linear index v = (i n1 + j) n2 + k;
//   * corner bits: bit a = +1 on axis a.  Every tetrahedron edge of the Kuhn (Freudenthal) split is a grid edge from its lower corner u in
//     one of 7 positive directions d = 0..6 = x, y, z, xy, xz, yz, xyz; edge id 7 u + d;
//   * one vertex per crossing edge, in edge-id order within the object: edge (u, d) has the index scan(u) - popc(mask(u)) +
//     popc(mask(u) & (2^d - 1)), mask(u) the crossing bits of u's outgoing edges and scan the inclusive scan of their counts.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/supnerf_hip.h"

namespace snr {

constexpr int GRID_MAX_N = 512;              // points per axis
constexpr int GRID_THREADS = 256;            // every geometry pass: one thread per point (or brick, or slot), 1-D

struct GridDims {
    int n0, n1, n2;              // points per axis
    long long nv, nc;            // points, cells per object
};

// The lattice of a launch over n_grids objects: min_n..GRID_MAX_N points per axis (2 where cells are walked, 1 for the density launches).
inline int grid_check(const snr_lattice* lat, int64_t n_grids, int min_n, GridDims& G) {
    if (!lat || n_grids < 0) return SNR_E_ARG;
    for (int a = 0; a < 3; ++a)
        if (lat->n[a] < min_n || lat->n[a] > GRID_MAX_N) return SNR_E_ARG;
    G.n0 = lat->n[0]; G.n1 = lat->n[1]; G.n2 = lat->n[2];
    G.nv = (long long)G.n0 * G.n1 * G.n2;
    G.nc = (long long)(G.n0 - 1) * (G.n1 - 1) * (G.n2 - 1);
    return SNR_OK;
}

inline unsigned grid_blocks(long long total) { return (unsigned)((total + GRID_THREADS - 1) / GRID_THREADS); }

__device__ __forceinline__ long long grid_thread() { return (long long)blockIdx.x * blockDim.x + threadIdx.x; }

// thread id -> object (returned) and index within it, per_obj entries per object
__device__ __forceinline__ long long grid_object(long long gid, long long per_obj, long long& rest) {
    const long long b = gid / per_obj;
    rest = gid - b * per_obj;
    return b;
}

// linear index -> coordinates on a lattice with n1 x n2 points in its two fast axes
__device__ __forceinline__ void grid_ijk(unsigned v, int n1, int n2, int& i, int& j, int& k) {
    const unsigned n12 = (unsigned)(n1 * n2);
    i = (int)(v / n12); j = (int)((v % n12) / (unsigned)n2); k = (int)(v % (unsigned)n2);
}

struct GridPoint {
    long long b;                 // object
    unsigned v;                  // linear index within the object
    int i, j, k;
};
__device__ __forceinline__ GridPoint grid_point(long long gid, long long per_obj, int n1, int n2) {
    GridPoint p;
    long long v;
    p.b = grid_object(gid, per_obj, v);
    p.v = (unsigned)v;
    grid_ijk(p.v, n1, n2, p.i, p.j, p.k);
    return p;
}

// direction d -> the corner bits it adds: 1, 2, 4, 3, 5, 6, 7 by nibble
__device__ __forceinline__ int kuhn_dir_bits(int d) { return (int)((0x7653421u >> (4 * d)) & 7u); }
// corner bits 1..7 -> direction: 0, 1, 3, 2, 4, 5, 6 by nibble
__device__ __forceinline__ int kuhn_dir_of(int bits) { return (int)((0x65423100u >> (4 * bits)) & 7u); }

__device__ __forceinline__ unsigned corner_off(int bits, int n1, int n2) {
    return (unsigned)((bits & 1) * n1 * n2 + ((bits >> 1) & 1) * n2 + ((bits >> 2) & 1));
}

// does point (i, j, k) + corner lie inside the grid?
__device__ __forceinline__ bool corner_inside(const GridDims& G, int i, int j, int k, int bits) {
    return i + (bits & 1) < G.n0 && j + ((bits >> 1) & 1) < G.n1 && k + ((bits >> 2) & 1) < G.n2;
}

// the object-local index of the vertex on edge (u, d); with d = 0, the first vertex of u's outgoing edges
__device__ __forceinline__ int edge_vertex_index(const unsigned char* __restrict__ mask, const int* __restrict__ escan, unsigned u, int d) {
    const unsigned m = mask[u];
    return escan[u] - __popc(m) + __popc(m & ((1u << d) - 1u));
}

// bit c = corner c of the cell with lower corner v is inside (value > level)
__device__ __forceinline__ unsigned cell_inside_bits(const float* __restrict__ f, unsigned v, int n1, int n2, float level) {
    unsigned in = 0;
    for (int c = 0; c < 8; ++c) in |= (unsigned)(f[v + corner_off(c, n1, n2)] > level) << c;
    return in;
}

}  // namespace snr
