// Mesh smoothing: vertex adjacency of a packed triangle mesh, the umbrella operator over it, Jacobi smoothing steps (Taubin 1995) and
// the operator's transpose for autograd.
//
// The rules are the header's (include/supnerf_hip.h, "Mesh smoothing"); tests/smooth_restatement.py restates them in numpy.  In short:
// two vertices of an object are neighbours iff a face names both; the adjacency is a CSR over all vertices of the call, neighbours
// ascending, with the number of faces on every edge beside it; U_i = (mean of the neighbours) - x_i in float64, the neighbours added in
// ascending order from 0.0; a step writes (float)(x_i + f U_i) into a second buffer.
//
// One pass over faces (keys; the caller sorts and compacts them into the CSR), then gathers only: one thread per vertex walks its own
// neighbour list.  The adjacency is symmetric, so the transpose is a gather over the same lists.  No LDS, no atomic but the bad-index
// flag, no launch reads what another thread of the same launch wrote: the same bits from run to run.
#include <climits>
#include "snr_packed_mesh.hpp"
#include "snr_host.hpp"

namespace snr {

constexpr int SMOOTH_KEY_BITS = 31;                    // the local target index of a key; the global source index sits above it
constexpr long long SMOOTH_MAX_VERTS = 1ll << 32;      // sum V of snr_smooth_edge_keys: (source << 31 | target) stays below INT64_MAX
constexpr int SMOOTH_CHUNK = 4;                        // channels one walk of a neighbour list sums side by side

// ---- rules 1 and 2: the six directed pairs of a face, each undirected edge of the face once per direction
__global__ void smooth_edge_keys_kernel(const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
                                        long long B, long long nV, long long nF, long long* __restrict__ key, int* bad) {
    const long long f = grid_thread();
    if (f >= nF) return;
    const MeshFace m = mesh_face(faces, voff, foff, B, nV, f);
    if (!m.ok) __hip_atomic_store(bad, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int i0 = m.idx[0], i1 = m.idx[1], i2 = m.idx[2];
    // edge k = (idx[k], idx[k + 1]); with a repeated index one edge has no length and the other two are the same pair: the later one goes
    const bool keep[3] = {m.ok && i0 != i1, m.ok && i1 != i2 && i2 != i0, m.ok && i2 != i0 && i2 != i1 && i0 != i1};
    for (int k = 0; k < 3; ++k) {
        const long long a = m.idx[k], b = m.idx[k == 2 ? 0 : k + 1];
        key[f * 6 + 2 * k] = keep[k] ? ((m.v0 + a) << SMOOTH_KEY_BITS) | b : LLONG_MAX;
        key[f * 6 + 2 * k + 1] = keep[k] ? ((m.v0 + b) << SMOOTH_KEY_BITS) | a : LLONG_MAX;
    }
}

// ---- rule 3: a vertex is a boundary (non-manifold) vertex iff one of its edges has one face (more than two)
__global__ void smooth_vertex_flags_kernel(const long long* __restrict__ nbr_start, const int* __restrict__ edge_faces, long long nV,
                                           long long nE, unsigned char* __restrict__ boundary, unsigned char* __restrict__ nonmanifold) {
    const long long g = grid_thread();
    if (g >= nV) return;
    const SmoothRing r = smooth_ring(nbr_start, g, nE);
    bool bd = false, nm = false;
    for (long long e = r.begin; e < r.end; ++e) {
        const int c = edge_faces[e];
        bd = bd || c == 1;
        nm = nm || c > 2;
    }
    boundary[g] = bd;
    nonmanifold[g] = nm;
}

// ---- rules 4, 5 and 7.  MODE: what a vertex writes from the sums over its neighbours
enum : int { SMOOTH_STEP = 0, SMOOTH_LAPLACIAN = 1, SMOOTH_TRANSPOSE = 2 };

template <int MODE>
__global__ void __launch_bounds__(GRID_THREADS) smooth_gather_kernel(const float* __restrict__ x, int C, const long long* __restrict__ nbr_start,
                                                                     const int* __restrict__ nbr, const long long* __restrict__ voff,
                                                                     long long B, long long nV, long long nE,
                                                                     const unsigned char* __restrict__ pinned, double factor,
                                                                     float* __restrict__ out) {
    const long long g = grid_thread();
    if (g >= nV) return;
    const MeshObject o = mesh_object(voff, mesh_entry_of(voff, B, g), nV);
    const SmoothRing r = smooth_ring(nbr_start, g, nE);
    const long long d = r.degree();
    const float* __restrict__ xi = x + g * C;
    float* __restrict__ oi = out + g * C;
    if (MODE == SMOOTH_STEP && (d == 0 || (pinned && pinned[g]))) {                 // rule 5: the same bits
        for (int c = 0; c < C; ++c) oi[c] = xi[c];
        return;
    }
    for (int c0 = 0; c0 < C; c0 += SMOOTH_CHUNK) {
        double s[SMOOTH_CHUNK];
        for (int k = 0; k < SMOOTH_CHUNK; ++k) s[k] = 0.0;
        for (long long e = r.begin; e < r.end; ++e) {                               // ascending: the order is the contract
            const int j = nbr[e];
            if (!mesh_index_ok(j, o.V)) continue;                                   // (an entry out of range adds nothing)
            const long long gj = o.v0 + j;
            const float* __restrict__ xj = x + gj * C + c0;
            if (MODE == SMOOTH_TRANSPOSE) {
                const double dj = (double)smooth_ring(nbr_start, gj, nE).degree();
#pragma unroll
                for (int k = 0; k < SMOOTH_CHUNK; ++k)
                    if (c0 + k < C) s[k] += (double)xj[k] / dj;
            } else {
#pragma unroll
                for (int k = 0; k < SMOOTH_CHUNK; ++k)
                    if (c0 + k < C) s[k] += (double)xj[k];
            }
        }
#pragma unroll
        for (int k = 0; k < SMOOTH_CHUNK; ++k) {
            if (c0 + k >= C) continue;
            const double xc = (double)xi[c0 + k];
            if (MODE == SMOOTH_TRANSPOSE) {
                oi[c0 + k] = (float)(d > 0 ? s[k] - xc : s[k]);
            } else {
                const double u = d > 0 ? s[k] / (double)d - xc : 0.0;
                oi[c0 + k] = MODE == SMOOTH_STEP ? (float)(xc + factor * u) : (float)u;
            }
        }
    }
}

// what snr_smooth_step and snr_smooth_laplacian check alike
inline int smooth_gather_args(const float* x, int C, const int64_t* nbr_start, const int32_t* nbr, const int64_t* vert_offset,
                              int64_t n_objects, int64_t n_verts, int64_t n_edges, const float* out, bool& nothing) {
    nothing = false;
    const int rc = packed_sizes(n_objects, n_verts, n_edges);
    if (rc != SNR_OK) return rc;
    if (C < 1 || C > PACKED_MAX_CHANNELS) return SNR_E_ARG;
    if (n_verts == 0) { nothing = true; return SNR_OK; }
    if (n_objects == 0 || !x || !out || !nbr_start || !vert_offset || (n_edges && !nbr)) return SNR_E_ARG;
    const uintptr_t a = (uintptr_t)x, b = (uintptr_t)out, bytes = (uintptr_t)n_verts * C * sizeof(float);
    if (a < b + bytes && b < a + bytes) return SNR_E_ARG;                           // a Jacobi step: the two buffers are apart
    return SNR_OK;
}

}  // namespace snr

using namespace snr;

extern "C" {

int snr_smooth_edge_keys(const int32_t* faces, const int64_t* vert_offset, const int64_t* face_offset, int64_t n_objects, int64_t n_verts,
                         int64_t n_faces, int64_t* key, int32_t* bad, void* stream) {
    const int rc = packed_sizes(n_objects, n_verts, n_faces);
    if (rc != SNR_OK) return rc;
    if (n_verts >= SMOOTH_MAX_VERTS || n_faces * 6 > PACKED_MAX_ITEMS) return SNR_E_UNSUPPORTED;
    if (!bad) return SNR_E_ARG;
    if (n_faces == 0) return SNR_OK;
    if (n_objects == 0 || !faces || !vert_offset || !face_offset || !key) return SNR_E_ARG;
    smooth_edge_keys_kernel<<<grid_blocks(n_faces), GRID_THREADS, 0, (hipStream_t)stream>>>(
        faces, (const long long*)vert_offset, (const long long*)face_offset, n_objects, n_verts, n_faces, (long long*)key, bad);
    return snr_check_launch_();
}

int snr_smooth_vertex_flags(const int64_t* nbr_start, const int32_t* edge_faces, int64_t n_verts, int64_t n_edges, uint8_t* boundary,
                            uint8_t* nonmanifold, void* stream) {
    const int rc = packed_sizes(0, n_verts, n_edges);
    if (rc != SNR_OK) return rc;
    if (n_verts == 0) return SNR_OK;
    if (!nbr_start || !boundary || !nonmanifold || (n_edges && !edge_faces)) return SNR_E_ARG;
    smooth_vertex_flags_kernel<<<grid_blocks(n_verts), GRID_THREADS, 0, (hipStream_t)stream>>>((const long long*)nbr_start, edge_faces, n_verts,
                                                                                              n_edges, boundary, nonmanifold);
    return snr_check_launch_();
}

int snr_smooth_step(const float* x_in, int n_channels, const int64_t* nbr_start, const int32_t* nbr, const int64_t* vert_offset,
                    int64_t n_objects, int64_t n_verts, int64_t n_edges, const uint8_t* pinned, double factor, float* x_out, void* stream) {
    bool nothing;
    const int rc = smooth_gather_args(x_in, n_channels, nbr_start, nbr, vert_offset, n_objects, n_verts, n_edges, x_out, nothing);
    if (rc != SNR_OK || nothing) return rc;
    smooth_gather_kernel<SMOOTH_STEP><<<grid_blocks(n_verts), GRID_THREADS, 0, (hipStream_t)stream>>>(
        x_in, n_channels, (const long long*)nbr_start, nbr, (const long long*)vert_offset, n_objects, n_verts, n_edges, pinned, factor, x_out);
    return snr_check_launch_();
}

int snr_smooth_laplacian(const float* x, int n_channels, const int64_t* nbr_start, const int32_t* nbr, const int64_t* vert_offset,
                         int64_t n_objects, int64_t n_verts, int64_t n_edges, int transpose, float* out, void* stream) {
    bool nothing;
    const int rc = smooth_gather_args(x, n_channels, nbr_start, nbr, vert_offset, n_objects, n_verts, n_edges, out, nothing);
    if (rc != SNR_OK) return rc;
    if (transpose != 0 && transpose != 1) return SNR_E_ARG;
    if (nothing) return SNR_OK;
    hipStream_t st = (hipStream_t)stream;
    const long long* ns = (const long long*)nbr_start;
    const long long* voff = (const long long*)vert_offset;
    if (transpose)
        smooth_gather_kernel<SMOOTH_TRANSPOSE><<<grid_blocks(n_verts), GRID_THREADS, 0, st>>>(x, n_channels, ns, nbr, voff, n_objects, n_verts,
                                                                                             n_edges, nullptr, 0.0, out);
    else
        smooth_gather_kernel<SMOOTH_LAPLACIAN><<<grid_blocks(n_verts), GRID_THREADS, 0, st>>>(x, n_channels, ns, nbr, voff, n_objects, n_verts,
                                                                                             n_edges, nullptr, 0.0, out);
    return snr_check_launch_();
}

}  // extern "C"
