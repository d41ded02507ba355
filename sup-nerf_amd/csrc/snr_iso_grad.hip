// Backward of the iso-surface: vertex gradients to the grid values they were interpolated from, and the grid points the surface touches
// compacted into a point list for the density backward.
//
// The rule is the header's (include/supnerf_hip.h, "Iso-surface backward"); tests/iso_grad_restatement.py restates it in numpy, and the
// output of these kernels is bit-identical to it.  Grid indexing, the edge directions and the vertex index of an edge are snr_grid.hpp's,
// shared with the forward.  In short: the vertex on crossing edge (u, d), va = f(u), vb = f(u + d), sits at
// c_a = lo_a + h_a (i_a + t d_a) with t = (level - va) / (vb - va), so for an upstream gradient g
//   s = sum over the axes a with d_a = 1 of g_a h_a (axis order, fp32),  w = s / ((vb - va) (vb - va)),
//   d f(u) += w (level - vb),  d f(u + d) += w (va - level).
// One thread per grid point GATHERS these terms, in a fixed order: its outgoing crossing edges d = 0..6 (its own edge_mask bits), then its
// incoming ones d = 0..6 (bit d of the point u - dir(d)).  No atomics: the result is the same bit for bit from run to run.
//
// Both kernels are memory-bound passes of one thread per grid point (or list slot), a few tens of bytes each through L2.
#include "snr_device.hpp"
#include "snr_grid.hpp"
#include "snr_host.hpp"

namespace snr {

// w of one crossing edge: s / ((vb - va) (vb - va)), s = sum of g_a h_a over the edge's axes in axis order
__device__ __forceinline__ float isog_weight(const float* __restrict__ g, int bits, const snr_lattice& lat, float va, float vb) {
    float s = 0.f;
    for (int a = 0; a < 3; ++a)
        if ((bits >> a) & 1) s = s + g[a] * lat.h[a];
    const float diff = vb - va;
    return s / (diff * diff);
}

__global__ void iso_grad_kernel(const float* __restrict__ grid, long long total, GridDims G, float level, snr_lattice lat,
                                const unsigned char* __restrict__ edge_mask, const int* __restrict__ edge_scan,
                                const long long* __restrict__ vert_offset, const float* __restrict__ d_verts, float* __restrict__ d_grid,
                                unsigned char* __restrict__ on_surface) {
    const long long gid = grid_thread();
    if (gid >= total) return;
    const GridPoint pt = grid_point(gid, G.nv, G.n1, G.n2);
    const long long b = pt.b;
    const unsigned v = pt.v;
    const float* f = grid + b * G.nv;
    const unsigned char* mask = edge_mask + b * G.nv;
    const int* escan = edge_scan + b * G.nv;
    const float* g = d_verts + vert_offset[b] * 3;       // the object's vertex gradients (object-local vertex indices)
    const float fu = f[v];
    float acc = 0.f;
    bool on = false;

    // ---- outgoing crossing edges (u = this point): its vertices in direction order, as iso_emit_kernel wrote them
    const unsigned m = mask[v];
    if (m) {
        int w = edge_vertex_index(mask, escan, v, 0);
        for (int d = 0; d < 7; ++d) {
            if (!((m >> d) & 1u)) continue;
            const int bits = kuhn_dir_bits(d);
            const float vb = f[v + corner_off(bits, G.n1, G.n2)];
            acc = acc + isog_weight(g + 3ll * w, bits, lat, fu, vb) * (level - vb);
            ++w;
        }
        on = true;
    }
    // ---- incoming crossing edges (u + dir(d) = this point)
    for (int d = 0; d < 7; ++d) {
        const int bits = kuhn_dir_bits(d);
        if (pt.i < (bits & 1) || pt.j < ((bits >> 1) & 1) || pt.k < ((bits >> 2) & 1)) continue;
        const unsigned p = v - corner_off(bits, G.n1, G.n2);
        if (!((mask[p] >> d) & 1u)) continue;
        const int w = edge_vertex_index(mask, escan, p, d);
        const float va = f[p];
        acc = acc + isog_weight(g + 3ll * w, bits, lat, va, fu) * (va - level);
        on = true;
    }
    d_grid[gid] = acc;
    if (on_surface) on_surface[gid] = on ? 1 : 0;
}

// One thread per (object, slot or grid point) over max(nv, points_per_obj) per object: a flagged grid point goes to slot scan - 1 of its
// object with its lattice coordinate (lo + h i: one multiply, one add) and its d f; slots from the object's count on are padding (lo, 0).
__global__ void iso_surface_points_kernel(const unsigned char* __restrict__ on_surface, const int* __restrict__ scan,
                                          const float* __restrict__ d_grid, long long total, long long per_obj, GridDims G, snr_lattice lat,
                                          long long points_per_obj, float* __restrict__ xyz, float* __restrict__ d_sig) {
    const long long gid = grid_thread();
    if (gid >= total) return;
    long long v;
    const long long b = grid_object(gid, per_obj, v);
    const long long row = b * G.nv;
    const long long out = b * points_per_obj;
    if (v < G.nv && on_surface[row + v]) {
        const long long s = (long long)scan[row + v] - 1;
        if (s < points_per_obj) {
            int ia[3];
            grid_ijk((unsigned)v, G.n1, G.n2, ia[0], ia[1], ia[2]);
            for (int a = 0; a < 3; ++a) xyz[(out + s) * 3 + a] = lat.lo[a] + lat.h[a] * (float)ia[a];
            d_sig[out + s] = d_grid[row + v];
        }
    }
    const long long count = scan[row + G.nv - 1];
    if (v >= count && v < points_per_obj) {
        for (int a = 0; a < 3; ++a) xyz[(out + v) * 3 + a] = lat.lo[a];
        d_sig[out + v] = 0.f;
    }
}

}  // namespace snr

using namespace snr;

extern "C" {

int snr_iso_grad(const float* grid, int64_t n_grids, const snr_lattice* lattice, float level, const uint8_t* edge_mask, const int32_t* edge_scan,
                 const int64_t* vert_offset, const float* d_verts, float* d_grid, uint8_t* on_surface, void* stream) {
    GridDims G;
    const int rc = grid_check(lattice, n_grids, 2, G);
    if (rc != SNR_OK) return rc;
    if (!grid || !edge_mask || !edge_scan || !vert_offset || !d_grid) return SNR_E_ARG;
    const long long total = n_grids * G.nv;
    if (total == 0) return SNR_OK;
    // (d_verts may be null when the surface is empty: no edge crosses, nothing is read from it)
    iso_grad_kernel<<<grid_blocks(total), GRID_THREADS, 0, (hipStream_t)stream>>>(grid, total, G, level, *lattice, edge_mask, edge_scan,
                                                                                   (const long long*)vert_offset, d_verts, d_grid, on_surface);
    return snr_check_launch_();
}

int snr_iso_surface_points(const uint8_t* on_surface, const int32_t* surface_scan, const float* d_grid, int64_t n_grids,
                           const snr_lattice* lattice, int64_t points_per_obj, float* xyz, float* d_sigmas, void* stream) {
    GridDims G;
    const int rc = grid_check(lattice, n_grids, 2, G);
    if (rc != SNR_OK) return rc;
    if (!on_surface || !surface_scan || !d_grid || points_per_obj < 0) return SNR_E_ARG;
    if (points_per_obj > 0 && (!xyz || !d_sigmas)) return SNR_E_ARG;
    const long long per_obj = G.nv > points_per_obj ? G.nv : points_per_obj;
    const long long total = n_grids * per_obj;
    if (total == 0) return SNR_OK;
    iso_surface_points_kernel<<<grid_blocks(total), GRID_THREADS, 0, (hipStream_t)stream>>>(on_surface, surface_scan, d_grid, total, per_obj, G,
                                                                                             *lattice, points_per_obj, xyz, d_sigmas);
    return snr_check_launch_();
}

}  // extern "C"
