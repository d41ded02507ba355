// Narrow-band density grids: the bookkeeping around the brick mode of the density decoder (snr_density_bricks), so that the decoder runs
// only on the bricks of 8^3 lattice points that the surface crosses.
//
// The rules are the header's (include/supnerf_hip.h, "Narrow band"); tests/band_restatement.py restates them in numpy.  In short:
//   * brick (I, J, K) owns the fine points [8I, 8I+8) x [8J, 8J+8) x [8K, 8K+8) inside the grid; its corners are the points (I..I+1, J..J+1,
//     K..K+1) of the coarse lattice (the fine one's points at multiples of 8, one more per axis past the far edge);
//   * classify: a brick is active when its 8 corners are not all on one side of the level (inside: value > level), when a corner lies
//     within `band` of the level, or when a corner is not finite.  Fill value: the largest corner when all 8 are inside, else the smallest
//     (for a one-sided brick the corner farthest from the level); NaN when a corner is not finite;
//   * state per brick: 0 = not evaluated (its points hold the fill value), s >= 1 = evaluated in round s - 1 (1: the first evaluation);
//   * seam: every grid edge of the iso kernels' 7 Kuhn directions (snr_grid.hpp: the same functions walk them) that crosses the level and
//     has an endpoint in a brick not yet evaluated activates the bricks that own its unevaluated endpoints.
//
// Every kernel is one thread per brick or per fine grid point and moves a few bytes per thread: memory-bound passes, small next to the
// decoder work they save.
#include "snr_device.hpp"
#include "snr_grid.hpp"
#include "snr_host.hpp"

namespace snr {

struct BandGrid : GridDims {     // the fine grid, and:
    int nb0, nb1, nb2;           // bricks per axis, ceil(n / 8); the coarse lattice has nb + 1 points per axis
    long long nbr, ncoarse;      // bricks, coarse points per object
};

__device__ __forceinline__ long long band_brick(const BandGrid& G, int i, int j, int k) {
    return ((long long)(i >> 3) * G.nb1 + (j >> 3)) * G.nb2 + (k >> 3);
}

__global__ void band_classify_kernel(const float* __restrict__ coarse, long long total, BandGrid G, float level, float band,
                                     int* __restrict__ state, float* __restrict__ fill) {
    const long long gid = grid_thread();
    if (gid >= total) return;
    const GridPoint p = grid_point(gid, G.nbr, G.nb1, G.nb2);        // (the bricks of an object are a lattice too)
    const int I = p.i, J = p.j, K = p.k;
    const float* c = coarse + p.b * G.ncoarse;
    int n_in = 0;
    bool finite = true, near = false;
    float lo = __builtin_inff(), hi = -__builtin_inff();
    for (int q = 0; q < 8; ++q) {
        const float v = c[((long long)(I + (q & 1)) * (G.nb1 + 1) + J + ((q >> 1) & 1)) * (G.nb2 + 1) + K + ((q >> 2) & 1)];
        n_in += v > level;
        finite = finite && isfinite(v);
        near = near || fabsf(v - level) <= band;
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    const bool active = !finite || near || (n_in != 0 && n_in != 8);
    state[gid] = active ? 1 : 0;
    fill[gid] = !finite ? __builtin_nanf("") : (n_in == 8 ? hi : lo);
}

__global__ void band_compact_kernel(const int* __restrict__ state, const int* __restrict__ scan, long long total, BandGrid G,
                                    int* __restrict__ bricks) {
    const long long gid = grid_thread();
    if (gid >= total || state[gid] != 1) return;
    const GridPoint p = grid_point(gid, G.nbr, G.nb1, G.nb2);
    int* o = bricks + (long long)(scan[gid] - 1) * 4;
    o[0] = (int)p.b; o[1] = p.i; o[2] = p.j; o[3] = p.k;
}

__global__ void band_fill_kernel(float* __restrict__ grid, long long total, BandGrid G, const int* __restrict__ state, const float* __restrict__ fill) {
    const long long gid = grid_thread();
    if (gid >= total) return;
    const GridPoint p = grid_point(gid, G.nv, G.n1, G.n2);
    const long long r = p.b * G.nbr + band_brick(G, p.i, p.j, p.k);
    if (state[r] == 0) grid[gid] = fill[r];
}

// Activate brick r of object b (state 0 -> stamp) once, and append it to the round's list.
__device__ __forceinline__ void band_activate(int* st, long long r, long long b, const BandGrid& G, int stamp, int* bricks, int* n_new) {
    if (st[r] != 0) return;                                   // (already activated: by an earlier round, or by another edge of this one)
    if (atomicCAS(st + r, 0, stamp) != 0) return;
    int* o = bricks + (long long)atomicAdd(n_new, 1) * 4;
    o[0] = (int)b;
    grid_ijk((unsigned)r, G.nb1, G.nb2, o[1], o[2], o[3]);
}

// One thread per grid point u: its <= 7 outgoing edges.  A brick counts as evaluated iff 1 <= state < stamp, so a brick this pass activates
// (state = stamp) still counts as unevaluated for the rest of the pass: the set of bricks activated does not depend on the threads' order.
__global__ void band_seam_kernel(const float* __restrict__ grid, long long total, BandGrid G, float level, int stamp, int* state,
                                 int* __restrict__ bricks, int* n_new) {
    const long long gid = grid_thread();
    if (gid >= total) return;
    const GridPoint p = grid_point(gid, G.nv, G.n1, G.n2);
    const long long b = p.b;
    const unsigned v = p.v;
    const int i = p.i, j = p.j, k = p.k;
    const float* f = grid + b * G.nv;
    int* st = state + b * G.nbr;
    const long long ru = band_brick(G, i, j, k);
    const int su = st[ru];
    const bool ev_u = su >= 1 && su < stamp;
    bool in0 = false, have_in0 = false;
#pragma unroll                                                 // (rolled, the 7 state loads wait for each other: 246 us against 171 at 256^3)
    for (int d = 0; d < 7; ++d) {
        const int bits = kuhn_dir_bits(d);
        if (!corner_inside(G, i, j, k, bits)) continue;
        const long long rw = band_brick(G, i + (bits & 1), j + ((bits >> 1) & 1), k + ((bits >> 2) & 1));
        const int sw = st[rw];
        const bool ev_w = sw >= 1 && sw < stamp;
        if (ev_u && ev_w) continue;                            // both ends exact: nothing to grow
        if (!have_in0) { in0 = f[v] > level; have_in0 = true; }
        if ((f[v + corner_off(bits, G.n1, G.n2)] > level) == in0) continue;
        if (!ev_u) band_activate(st, ru, b, G, stamp, bricks, n_new);
        if (!ev_w) band_activate(st, rw, b, G, stamp, bricks, n_new);
    }
}

// grid_check, and the brick counts of the lattice
static int band_dims(const snr_lattice* lat, int64_t n_grids, BandGrid& G) {
    const int rc = grid_check(lat, n_grids, 2, G);
    if (rc != SNR_OK) return rc;
    G.nb0 = (G.n0 + 7) / 8; G.nb1 = (G.n1 + 7) / 8; G.nb2 = (G.n2 + 7) / 8;
    G.nbr = (long long)G.nb0 * G.nb1 * G.nb2;
    G.ncoarse = (long long)(G.nb0 + 1) * (G.nb1 + 1) * (G.nb2 + 1);
    return SNR_OK;
}

}  // namespace snr

using namespace snr;

extern "C" {

int snr_band_classify(const float* coarse, int64_t n_grids, const snr_lattice* lattice, float level, float band, int32_t* state, float* fill,
                      void* stream) {
    BandGrid G;
    const int rc = band_dims(lattice, n_grids, G);
    if (rc != SNR_OK) return rc;
    if (!coarse || !state || !fill || !(band >= 0.f)) return SNR_E_ARG;
    const long long total = n_grids * G.nbr;
    if (total == 0) return SNR_OK;
    band_classify_kernel<<<grid_blocks(total), GRID_THREADS, 0, (hipStream_t)stream>>>(coarse, total, G, level, band, state, fill);
    return snr_check_launch_();
}

int snr_band_compact(const int32_t* state, const int32_t* scan, int64_t n_grids, const snr_lattice* lattice, int32_t* bricks, void* stream) {
    BandGrid G;
    const int rc = band_dims(lattice, n_grids, G);
    if (rc != SNR_OK) return rc;
    if (!state || !scan || !bricks) return SNR_E_ARG;
    const long long total = n_grids * G.nbr;
    if (total == 0) return SNR_OK;
    band_compact_kernel<<<grid_blocks(total), GRID_THREADS, 0, (hipStream_t)stream>>>(state, scan, total, G, bricks);
    return snr_check_launch_();
}

int snr_band_fill(float* grid, int64_t n_grids, const snr_lattice* lattice, const int32_t* state, const float* fill, void* stream) {
    BandGrid G;
    const int rc = band_dims(lattice, n_grids, G);
    if (rc != SNR_OK) return rc;
    if (!grid || !state || !fill) return SNR_E_ARG;
    const long long total = n_grids * G.nv;
    if (total == 0) return SNR_OK;
    band_fill_kernel<<<grid_blocks(total), GRID_THREADS, 0, (hipStream_t)stream>>>(grid, total, G, state, fill);
    return snr_check_launch_();
}

int snr_band_seam(const float* grid, int64_t n_grids, const snr_lattice* lattice, float level, int32_t stamp, int32_t* state, int32_t* bricks,
                  int32_t* n_new, void* stream) {
    BandGrid G;
    const int rc = band_dims(lattice, n_grids, G);
    if (rc != SNR_OK) return rc;
    if (!grid || !state || !bricks || !n_new || stamp < 2) return SNR_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(n_new, 0, sizeof(int32_t), st) != hipSuccess) return snr_check_launch_();
    const long long total = n_grids * G.nv;
    if (total == 0) return SNR_OK;
    band_seam_kernel<<<grid_blocks(total), GRID_THREADS, 0, st>>>(grid, total, G, level, stamp, state, bricks, n_new);
    return snr_check_launch_();
}

}  // extern "C"
