// Backward of the iso-surface: vertex gradients to the grid values they were interpolated from, and the grid points the surface touches
// compacted into a point list for the density backward.
//
// The rule is the header's (include/supnerf_hip.h, "Iso-surface backward"); tests/iso_grad_restatement.py restates it in numpy, and the
// output of these kernels is bit-identical to it.  In short: the vertex on crossing edge (u, d), va = f(u), vb = f(u + d), sits at
// c_a = lo_a + h_a (i_a + t d_a) with t = (level - va) / (vb - va), so for an upstream gradient g
//   s = sum over the axes a with d_a = 1 of g_a h_a (axis order, fp32),  w = s / ((vb - va) (vb - va)),
//   d f(u) += w (level - vb),  d f(u + d) += w (va - level).
// One thread per grid point GATHERS these terms, in a fixed order: its outgoing crossing edges d = 0..6 (its own edge_mask bits), then its
// incoming ones d = 0..6 (bit d of the point u - dir(d)).  No atomics: the result is the same bit for bit from run to run.
//
// Both kernels are memory-bound passes of one thread per grid point (or list slot), a few tens of bytes each through L2.
#include "snr_device.hpp"
#include "snr_host.hpp"

namespace snr {

constexpr int ISO_GRAD_MAX_N = 512;

struct IsoGradGrid {
    int n0, n1, n2;
    long long nv;                // grid points per object
};

// direction d (0..6 = x, y, z, xy, xz, yz, xyz) -> the corner bits it adds (bit a = +1 on axis a): 1, 2, 4, 3, 5, 6, 7 by nibble
__device__ __forceinline__ int isog_dir_bits(int d) { return (int)((0x7653421u >> (4 * d)) & 7u); }

__device__ __forceinline__ unsigned isog_off(int bits, int n1, int n2) {
    return (unsigned)((bits & 1) * n1 * n2 + ((bits >> 1) & 1) * n2 + ((bits >> 2) & 1));
}

// w of one crossing edge: s / ((vb - va) (vb - va)), s = sum of g_a h_a over the edge's axes in axis order
__device__ __forceinline__ float isog_weight(const float* __restrict__ g, int bits, const snr_lattice& lat, float va, float vb) {
    float s = 0.f;
    for (int a = 0; a < 3; ++a)
        if ((bits >> a) & 1) s = s + g[a] * lat.h[a];
    const float diff = vb - va;
    return s / (diff * diff);
}

__global__ void iso_grad_kernel(const float* __restrict__ grid, long long total, IsoGradGrid G, float level, snr_lattice lat,
                                const unsigned char* __restrict__ edge_mask, const int* __restrict__ edge_scan,
                                const long long* __restrict__ vert_offset, const float* __restrict__ d_verts, float* __restrict__ d_grid,
                                unsigned char* __restrict__ on_surface) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const long long b = gid / G.nv;
    const unsigned v = (unsigned)(gid - b * G.nv);
    const unsigned n12 = (unsigned)(G.n1 * G.n2);
    const int i = (int)(v / n12), j = (int)((v % n12) / (unsigned)G.n2), k = (int)(v % (unsigned)G.n2);
    const float* f = grid + b * G.nv;
    const unsigned char* mask = edge_mask + b * G.nv;
    const int* escan = edge_scan + b * G.nv;
    const float* g = d_verts + vert_offset[b] * 3;       // the object's vertex gradients (object-local vertex indices)
    const float fu = f[v];
    float acc = 0.f;
    bool on = false;

    // ---- outgoing crossing edges (u = this point): the vertices escan - popc(m) ... in direction order, as iso_emit_kernel wrote them
    const unsigned m = mask[v];
    if (m) {
        int w = escan[v] - __popc(m);
        for (int d = 0; d < 7; ++d) {
            if (!((m >> d) & 1u)) continue;
            const int bits = isog_dir_bits(d);
            const float vb = f[v + isog_off(bits, G.n1, G.n2)];
            acc = acc + isog_weight(g + 3ll * w, bits, lat, fu, vb) * (level - vb);
            ++w;
        }
        on = true;
    }
    // ---- incoming crossing edges (u + dir(d) = this point)
    for (int d = 0; d < 7; ++d) {
        const int bits = isog_dir_bits(d);
        if (i < (bits & 1) || j < ((bits >> 1) & 1) || k < ((bits >> 2) & 1)) continue;
        const unsigned p = v - isog_off(bits, G.n1, G.n2);
        const unsigned mp = mask[p];
        if (!((mp >> d) & 1u)) continue;
        const int w = escan[p] - __popc(mp) + __popc(mp & ((1u << d) - 1u));
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
                                          const float* __restrict__ d_grid, long long total, long long per_obj, IsoGradGrid G, snr_lattice lat,
                                          long long points_per_obj, float* __restrict__ xyz, float* __restrict__ d_sig) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const long long b = gid / per_obj;
    const long long v = gid - b * per_obj;
    const long long row = b * G.nv;
    const long long out = b * points_per_obj;
    if (v < G.nv && on_surface[row + v]) {
        const long long s = (long long)scan[row + v] - 1;
        if (s < points_per_obj) {
            const unsigned n12 = (unsigned)(G.n1 * G.n2), u = (unsigned)v;
            const int ia[3] = {(int)(u / n12), (int)((u % n12) / (unsigned)G.n2), (int)(u % (unsigned)G.n2)};
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

static int iso_grad_check(const snr_lattice* lat, int64_t n_grids, IsoGradGrid& G) {
    if (!lat || n_grids < 0) return SNR_E_ARG;
    for (int a = 0; a < 3; ++a)
        if (lat->n[a] < 2 || lat->n[a] > ISO_GRAD_MAX_N) return SNR_E_ARG;
    G.n0 = lat->n[0]; G.n1 = lat->n[1]; G.n2 = lat->n[2];
    G.nv = (long long)G.n0 * G.n1 * G.n2;
    return SNR_OK;
}

}  // namespace snr

using namespace snr;

extern "C" {

int snr_iso_grad(const float* grid, int64_t n_grids, const snr_lattice* lattice, float level, const uint8_t* edge_mask, const int32_t* edge_scan,
                 const int64_t* vert_offset, const float* d_verts, float* d_grid, uint8_t* on_surface, void* stream) {
    IsoGradGrid G;
    const int rc = iso_grad_check(lattice, n_grids, G);
    if (rc != SNR_OK) return rc;
    if (!grid || !edge_mask || !edge_scan || !vert_offset || !d_grid) return SNR_E_ARG;
    const long long total = n_grids * G.nv;
    if (total == 0) return SNR_OK;
    // (d_verts may be null when the surface is empty: no edge crosses, nothing is read from it)
    iso_grad_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(grid, total, G, level, *lattice, edge_mask, edge_scan,
                                                                                       (const long long*)vert_offset, d_verts, d_grid,
                                                                                       on_surface);
    return snr_check_launch_();
}

int snr_iso_surface_points(const uint8_t* on_surface, const int32_t* surface_scan, const float* d_grid, int64_t n_grids,
                           const snr_lattice* lattice, int64_t points_per_obj, float* xyz, float* d_sigmas, void* stream) {
    IsoGradGrid G;
    const int rc = iso_grad_check(lattice, n_grids, G);
    if (rc != SNR_OK) return rc;
    if (!on_surface || !surface_scan || !d_grid || points_per_obj < 0) return SNR_E_ARG;
    if (points_per_obj > 0 && (!xyz || !d_sigmas)) return SNR_E_ARG;
    const long long per_obj = G.nv > points_per_obj ? G.nv : points_per_obj;
    const long long total = n_grids * per_obj;
    if (total == 0) return SNR_OK;
    iso_surface_points_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(on_surface, surface_scan, d_grid, total, per_obj,
                                                                                                 G, *lattice, points_per_obj, xyz, d_sigmas);
    return snr_check_launch_();
}

}  // extern "C"
