// The grid of "Mesh distance" D3 (include/supnerf_hip.h), stated once for the kernels that build and walk it: snr_nearest.hip (the
// closest-point search) and snr_inside.hip (the winding number, whose rule W5 needs the very cell function the lists were built with).
// Functions only (see snr_grid.hpp).
#pragma once
#include "snr_packed_mesh.hpp"

namespace snr {

constexpr int NEAREST_MAX_CELLS = 256;                 // cells per axis (D3)

__device__ __forceinline__ void nearest_flag(int* bad) { __hip_atomic_store(bad, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ bool nearest_finite(float x) { return fabsf(x) <= 3.4028234e38f; }            // (false for NaN)

// ---- D3: the grid of object b
struct NearestGrid {
    bool ok;                     // h > 0 and finite, finite bounds, hi >= lo, and cell_offset holds exactly this grid's cells
    double lo[3], h, extent;     // the anchor, the cell edge and the largest extent over the axes, widened
    int n[3];                    // cells per axis
    long long c0;                // the global id of the object's cell 0
};
__device__ __forceinline__ NearestGrid nearest_grid(const float* __restrict__ cell, const float* __restrict__ grid_lo,
                                                    const float* __restrict__ grid_hi, const long long* __restrict__ cell_offset,
                                                    long long b, long long n_cells) {
    NearestGrid g;
    const float hf = cell[b];
    g.ok = hf > 0.f && nearest_finite(hf);
    g.h = (double)hf;
    g.extent = 0.0;
    long long cells = 1;
    for (int a = 0; a < 3; ++a) {
        const float lo = grid_lo[b * 3 + a], hi = grid_hi[b * 3 + a];
        g.ok = g.ok && nearest_finite(lo) && nearest_finite(hi) && hi >= lo;
        g.lo[a] = (double)lo;
        const double e = (double)hi - (double)lo;
        g.extent = e > g.extent ? e : g.extent;
        const double q = ceil(e / g.h);
        g.n[a] = q >= 1.0 ? (q >= (double)NEAREST_MAX_CELLS ? NEAREST_MAX_CELLS : (int)q) : 1;               // (a NaN gives 1)
        cells *= g.n[a];
    }
    g.c0 = cell_offset[b];
    g.ok = g.ok && g.c0 >= 0 && cell_offset[b + 1] - g.c0 == cells && g.c0 + cells <= n_cells;
    return g;
}
// the cell of a coordinate on axis a: clamp(floor((x - lo) / h), 0, n - 1); a NaN gives 0
__device__ __forceinline__ int nearest_cell_of(const NearestGrid& g, int a, double x) {
    const double t = floor((x - g.lo[a]) / g.h);
    return t >= 1.0 ? (t >= (double)(g.n[a] - 1) ? g.n[a] - 1 : (int)t) : 0;
}

}  // namespace snr
