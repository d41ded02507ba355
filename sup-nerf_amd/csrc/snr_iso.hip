// Iso-surface of density grids: marching tetrahedra on the Kuhn (Freudenthal) split of every cell, two passes around a caller-side scan.
//
// The rule set is the header's (include/supnerf_hip.h, "Geometry"); tests/iso_restatement.py restates it step by step in numpy, and the
// output of these kernels is bit-identical to it.  In short:
//   * corner (bit a = +1 on axis a) of cell v000; the 6 tetrahedra v000 -> v000 + e_a -> v000 + e_a + e_b -> v111, permutations (a, b, c) in
//     the order 012, 021, 102, 120, 201, 210.  Their orientation is the permutation's sign: det(e_a, e_b, e_c).
//   * every tetrahedron edge is a grid edge from its lower corner u in one of 7 positive directions (x, y, z, xy, xz, yz, xyz): neighbouring
//     cells use the same face diagonals, so they share vertices exactly and the surface is closed wherever it does not meet the grid's border.
//   * inside: value > level.  One vertex per crossing edge, ordered by edge id 7 u + d; its index is base(u) + popcount(mask(u) & (2^d - 1)).
//   * triangles: winding from the tetrahedron's orientation and its case, never from geometry (a degenerate triangle has no normal).
//
// One thread per grid vertex in both passes: it owns the vertex's <= 7 outgoing edges and, when it is a cell's lower corner, that cell.
// The work is a few hundred bytes per grid point through L2 -- small next to the decoder launch that made the grid.
#include "snr_device.hpp"
#include "snr_host.hpp"

namespace snr {

constexpr int ISO_MAX_N = 512;
__constant__ unsigned char ISO_DIR_BITS[7] = {1, 2, 4, 3, 5, 6, 7};           // direction d -> the corner bits it adds
__constant__ signed char ISO_DIR_OF[8] = {-1, 0, 1, 3, 2, 4, 5, 6};            // corner bits -> direction
__constant__ unsigned char ISO_PERM[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
__constant__ bool ISO_POSITIVE[6] = {true, false, false, true, true, false};
// inside set of one tetrahedron vertex i (or outside set of one, with 3 inside): an even permutation (i, j, k, l) of (0, 1, 2, 3)
__constant__ unsigned char ISO_EVEN1[4][4] = {{0, 1, 2, 3}, {1, 0, 3, 2}, {2, 0, 1, 3}, {3, 0, 2, 1}};
// two inside, case bits s (bit p = tetrahedron vertex p inside): an even permutation (i, j, k, l) with {i, j} inside, i < j
__constant__ unsigned char ISO_EVEN2[16][4] = {
    {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 1, 2, 3}, {0, 0, 0, 0}, {0, 2, 3, 1}, {1, 2, 0, 3}, {0, 0, 0, 0},
    {0, 0, 0, 0}, {0, 3, 1, 2}, {1, 3, 2, 0}, {0, 0, 0, 0}, {2, 3, 0, 1}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};

struct IsoGrid {
    int nx, ny, nz;
    long long nv, nc;            // grid vertices, cells per object
};

__device__ __forceinline__ int iso_tri_count(int s) {
    const int n = __popc(s);
    return (n == 1 || n == 3) ? 1 : (n == 2 ? 2 : 0);
}

__device__ __forceinline__ unsigned corner_off(int bits, int ny, int nz) {
    return (unsigned)((bits & 1) * ny * nz + ((bits >> 1) & 1) * nz + ((bits >> 2) & 1));
}

__global__ void iso_count_kernel(const float* __restrict__ grid, long long total, IsoGrid G, float level, unsigned char* __restrict__ tri_count,
                                 unsigned char* __restrict__ edge_mask, unsigned char* __restrict__ edge_count) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const long long b = gid / G.nv;
    const unsigned v = (unsigned)(gid - b * G.nv);
    const unsigned nyz = (unsigned)(G.ny * G.nz);
    const int i = (int)(v / nyz), j = (int)((v % nyz) / (unsigned)G.nz), k = (int)(v % (unsigned)G.nz);
    const float* f = grid + b * G.nv;
    const bool in0 = f[v] > level;
    unsigned m = 0;
    for (int d = 0; d < 7; ++d) {
        const int bits = ISO_DIR_BITS[d];
        if (i + (bits & 1) < G.nx && j + ((bits >> 1) & 1) < G.ny && k + ((bits >> 2) & 1) < G.nz)
            if ((f[v + corner_off(bits, G.ny, G.nz)] > level) != in0) m |= 1u << d;
    }
    edge_mask[gid] = (unsigned char)m;
    edge_count[gid] = (unsigned char)__popc(m);
    if (i < G.nx - 1 && j < G.ny - 1 && k < G.nz - 1) {
        unsigned in = 0;
        for (int c = 0; c < 8; ++c) in |= (unsigned)(f[v + corner_off(c, G.ny, G.nz)] > level) << c;
        int n = 0;
        for (int t = 0; t < 6; ++t) {
            const int c1 = 1 << ISO_PERM[t][0], c2 = c1 | (1 << ISO_PERM[t][1]);
            const int s = (int)((in & 1) | (((in >> c1) & 1) << 1) | (((in >> c2) & 1) << 2) | (((in >> 7) & 1) << 3));
            n += iso_tri_count(s);
        }
        const long long cell = ((long long)i * (G.ny - 1) + j) * (G.nz - 1) + k;
        tri_count[b * G.nc + cell] = (unsigned char)n;
    }
}

struct TetCtx {
    const unsigned char* mask;   // the object's edge masks
    const int* escan;            // the object's inclusive edge-count scan
    unsigned v;                  // the cell's lower corner
    int ny, nz;
    int corner[4];               // corner bits of the tetrahedron's vertices 0..3 (nested: corner[p] is a subset of corner[q] for p < q)
};
// edge between tetrahedron vertices p < q: (edge id, vertex index within the object)
__device__ __forceinline__ void tet_edge(const TetCtx& c, int p, int q, long long& id, int& vid) {
    if (p > q) { const int x = p; p = q; q = x; }
    const unsigned u = c.v + corner_off(c.corner[p], c.ny, c.nz);
    const int d = ISO_DIR_OF[c.corner[q] ^ c.corner[p]];
    const unsigned m = c.mask[u];
    id = 7ll * u + d;
    vid = c.escan[u] - __popc(m) + __popc(m & ((1u << d) - 1u));
}

__global__ void iso_emit_kernel(const float* __restrict__ grid, long long total, IsoGrid G, float level, snr_lattice lat,
                                const unsigned char* __restrict__ edge_mask, const int* __restrict__ edge_scan, const int* __restrict__ tri_scan,
                                const long long* __restrict__ vert_offset, const long long* __restrict__ tri_offset, float* __restrict__ verts,
                                int* __restrict__ faces) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const long long b = gid / G.nv;
    const unsigned v = (unsigned)(gid - b * G.nv);
    const unsigned nyz = (unsigned)(G.ny * G.nz);
    const int i = (int)(v / nyz), j = (int)((v % nyz) / (unsigned)G.nz), k = (int)(v % (unsigned)G.nz);
    const float* f = grid + b * G.nv;
    const unsigned char* mask = edge_mask + b * G.nv;
    const int* escan = edge_scan + b * G.nv;

    // ---- the vertices of this grid vertex's crossing edges, in direction order
    const unsigned m = mask[v];
    if (m) {
        const float va = f[v];
        const int ia[3] = {i, j, k};
        long long w = vert_offset[b] + escan[v] - __popc(m);
        for (int d = 0; d < 7; ++d) {
            if (!((m >> d) & 1u)) continue;
            const int bits = ISO_DIR_BITS[d];
            const float vb = f[v + corner_off(bits, G.ny, G.nz)];
            const float t = (level - va) / (vb - va);
            for (int a = 0; a < 3; ++a) verts[w * 3 + a] = lat.lo[a] + lat.h[a] * ((float)ia[a] + t * (float)((bits >> a) & 1));
            ++w;
        }
    }

    // ---- the triangles of the cell whose lower corner this is
    if (i >= G.nx - 1 || j >= G.ny - 1 || k >= G.nz - 1) return;
    unsigned in = 0;
    for (int c = 0; c < 8; ++c) in |= (unsigned)(f[v + corner_off(c, G.ny, G.nz)] > level) << c;
    if (in == 0 || in == 0xffu) return;
    const long long cell = ((long long)i * (G.ny - 1) + j) * (G.nz - 1) + k;
    const int n_here = [&] {
        int n = 0;
        for (int t = 0; t < 6; ++t) {
            const int c1 = 1 << ISO_PERM[t][0], c2 = c1 | (1 << ISO_PERM[t][1]);
            n += iso_tri_count((int)((in & 1) | (((in >> c1) & 1) << 1) | (((in >> c2) & 1) << 2) | (((in >> 7) & 1) << 3)));
        }
        return n;
    }();
    long long w = tri_offset[b] + tri_scan[b * G.nc + cell] - n_here;
    TetCtx c;
    c.mask = mask; c.escan = escan; c.v = v; c.ny = G.ny; c.nz = G.nz;
    for (int t = 0; t < 6; ++t) {
        c.corner[0] = 0;
        c.corner[1] = 1 << ISO_PERM[t][0];
        c.corner[2] = c.corner[1] | (1 << ISO_PERM[t][1]);
        c.corner[3] = 7;
        int s = 0;
        for (int p = 0; p < 4; ++p) s |= (int)((in >> c.corner[p]) & 1u) << p;
        const int n = __popc(s);
        const bool pos = ISO_POSITIVE[t];
        long long id[4];
        int vid[4];
        if (n == 1 || n == 3) {
            // the lone vertex i (inside for n = 1, outside for n = 3); (i, j, k, l) even: (ij, ik, il) faces away from i on a positive tetrahedron
            const int lone = __ffs(n == 1 ? s : (~s & 15)) - 1;
            const unsigned char* e = ISO_EVEN1[lone];
            tet_edge(c, e[0], e[1], id[0], vid[0]);
            tet_edge(c, e[0], e[2], id[1], vid[1]);
            tet_edge(c, e[0], e[3], id[2], vid[2]);
            const bool keep = pos == (n == 1);
            int* o = faces + w * 3;
            o[0] = vid[0]; o[1] = keep ? vid[1] : vid[2]; o[2] = keep ? vid[2] : vid[1];
            ++w;
        } else if (n == 2) {
            // quad (ik, il, jl, jk) of the even (i, j, k, l), {i, j} inside: faces from {i, j} to {k, l} on a positive tetrahedron
            const unsigned char* e = ISO_EVEN2[s];
            tet_edge(c, e[0], e[2], id[0], vid[0]);
            if (pos) {
                tet_edge(c, e[0], e[3], id[1], vid[1]);
                tet_edge(c, e[1], e[2], id[3], vid[3]);
            } else {
                tet_edge(c, e[1], e[2], id[1], vid[1]);
                tet_edge(c, e[0], e[3], id[3], vid[3]);
            }
            tet_edge(c, e[1], e[3], id[2], vid[2]);
            int mq = 0;
            for (int q = 1; q < 4; ++q)
                if (id[q] < id[mq]) mq = q;
            int* o = faces + w * 3;
            o[0] = vid[mq]; o[1] = vid[(mq + 1) & 3]; o[2] = vid[(mq + 2) & 3];
            o[3] = vid[mq]; o[4] = vid[(mq + 2) & 3]; o[5] = vid[(mq + 3) & 3];
            w += 2;
        }
    }
}

static int iso_check(const snr_lattice* lat, int64_t n_grids, IsoGrid& G) {
    if (!lat || n_grids < 0) return SNR_E_ARG;
    for (int a = 0; a < 3; ++a)
        if (lat->n[a] < 2 || lat->n[a] > ISO_MAX_N) return SNR_E_ARG;
    G.nx = lat->n[0]; G.ny = lat->n[1]; G.nz = lat->n[2];
    G.nv = (long long)G.nx * G.ny * G.nz;
    G.nc = (long long)(G.nx - 1) * (G.ny - 1) * (G.nz - 1);
    return SNR_OK;
}

}  // namespace snr

using namespace snr;

extern "C" {

int snr_iso_count(const float* grid, int64_t n_grids, const snr_lattice* lattice, float level, uint8_t* tri_count, uint8_t* edge_mask,
                  uint8_t* edge_count, void* stream) {
    IsoGrid G;
    const int rc = iso_check(lattice, n_grids, G);
    if (rc != SNR_OK) return rc;
    if (!grid || !tri_count || !edge_mask || !edge_count) return SNR_E_ARG;
    const long long total = n_grids * G.nv;
    if (total == 0) return SNR_OK;
    iso_count_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(grid, total, G, level, tri_count, edge_mask, edge_count);
    return snr_check_launch_();
}

int snr_iso_emit(const float* grid, int64_t n_grids, const snr_lattice* lattice, float level, const uint8_t* edge_mask, const int32_t* edge_scan,
                 const int32_t* tri_scan, const int64_t* vert_offset, const int64_t* tri_offset, float* verts, int32_t* faces, void* stream) {
    IsoGrid G;
    const int rc = iso_check(lattice, n_grids, G);
    if (rc != SNR_OK) return rc;
    if (!grid || !edge_mask || !edge_scan || !tri_scan || !vert_offset || !tri_offset) return SNR_E_ARG;
    const long long total = n_grids * G.nv;
    if (total == 0) return SNR_OK;
    // (verts / faces may be null when the scans say the surface is empty: nothing is then written)
    iso_emit_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(grid, total, G, level, *lattice, edge_mask, edge_scan, tri_scan,
                                                                                       (const long long*)vert_offset, (const long long*)tri_offset,
                                                                                       verts, faces);
    return snr_check_launch_();
}

}  // extern "C"
