// Iso-surface of density grids: marching tetrahedra on the Kuhn (Freudenthal) split of every cell, two passes around a caller-side scan.
//
// The rule set is the header's (include/supnerf_hip.h, "Geometry"); tests/iso_restatement.py restates it step by step in numpy, and the
// output of these kernels is bit-identical to it.  Grid indexing, the 7 edge directions and the vertex index are snr_grid.hpp's; here:
//   * the 6 tetrahedra v000 -> v000 + e_a -> v000 + e_a + e_b -> v111 of a cell, permutations (a, b, c) in the order 012, 021, 102, 120,
//     201, 210.  Their orientation is the permutation's sign: det(e_a, e_b, e_c).  Neighbouring cells use the same face diagonals, so they
//     share vertices exactly and the surface is closed wherever it does not meet the grid's border.
//   * inside: value > level.  The vertex on a crossing edge sits at t = (level - va) / (vb - va).
//   * triangles: winding from the tetrahedron's orientation and its case, never from geometry (a degenerate triangle has no normal).
//
// One thread per grid vertex in both passes: it owns the vertex's <= 7 outgoing edges and, when it is a cell's lower corner, that cell.
// The work is a few hundred bytes per grid point through L2 -- small next to the decoder launch that made the grid.
#include "snr_device.hpp"
#include "snr_grid.hpp"
#include "snr_host.hpp"

namespace snr {

__constant__ unsigned char ISO_PERM[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
__constant__ bool ISO_POSITIVE[6] = {true, false, false, true, true, false};
// inside set of one tetrahedron vertex i (or outside set of one, with 3 inside): an even permutation (i, j, k, l) of (0, 1, 2, 3)
__constant__ unsigned char ISO_EVEN1[4][4] = {{0, 1, 2, 3}, {1, 0, 3, 2}, {2, 0, 1, 3}, {3, 0, 2, 1}};
// two inside, case bits s (bit p = tetrahedron vertex p inside): an even permutation (i, j, k, l) with {i, j} inside, i < j
__constant__ unsigned char ISO_EVEN2[16][4] = {
    {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 1, 2, 3}, {0, 0, 0, 0}, {0, 2, 3, 1}, {1, 2, 0, 3}, {0, 0, 0, 0},
    {0, 0, 0, 0}, {0, 3, 1, 2}, {1, 3, 2, 0}, {0, 0, 0, 0}, {2, 3, 0, 1}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};

// corner bits of vertices 1 and 2 of tetrahedron t (vertex 0 is corner 0, vertex 3 corner 7: nested)
__device__ __forceinline__ void tet_corners(int t, int& c1, int& c2) {
    c1 = 1 << ISO_PERM[t][0];
    c2 = c1 | (1 << ISO_PERM[t][1]);
}

// triangles of a cell with inside bits `in`: per tetrahedron 1 with one or three vertices inside, 2 with two
__device__ __forceinline__ int cell_tri_count(unsigned in) {
    int n = 0;
    for (int t = 0; t < 6; ++t) {
        int c1, c2;
        tet_corners(t, c1, c2);
        const int inside = __popc((in & 1) | (((in >> c1) & 1) << 1) | (((in >> c2) & 1) << 2) | (((in >> 7) & 1) << 3));
        n += (inside == 1 || inside == 3) ? 1 : (inside == 2 ? 2 : 0);
    }
    return n;
}

__device__ __forceinline__ long long cell_index(const GridDims& G, int i, int j, int k) {
    return ((long long)i * (G.n1 - 1) + j) * (G.n2 - 1) + k;
}

__global__ void iso_count_kernel(const float* __restrict__ grid, long long total, GridDims G, float level, unsigned char* __restrict__ tri_count,
                                 unsigned char* __restrict__ edge_mask, unsigned char* __restrict__ edge_count) {
    const long long gid = grid_thread();
    if (gid >= total) return;
    const GridPoint p = grid_point(gid, G.nv, G.n1, G.n2);
    const float* f = grid + p.b * G.nv;
    const bool in0 = f[p.v] > level;
    unsigned m = 0;
    for (int d = 0; d < 7; ++d) {
        const int bits = kuhn_dir_bits(d);
        if (corner_inside(G, p.i, p.j, p.k, bits))
            if ((f[p.v + corner_off(bits, G.n1, G.n2)] > level) != in0) m |= 1u << d;
    }
    edge_mask[gid] = (unsigned char)m;
    edge_count[gid] = (unsigned char)__popc(m);
    if (corner_inside(G, p.i, p.j, p.k, 7))
        tri_count[p.b * G.nc + cell_index(G, p.i, p.j, p.k)] = (unsigned char)cell_tri_count(cell_inside_bits(f, p.v, G.n1, G.n2, level));
}

struct TetCtx {
    const unsigned char* mask;   // the object's edge masks
    const int* escan;            // the object's inclusive edge-count scan
    unsigned v;                  // the cell's lower corner
    int n1, n2;
    int corner[4];               // corner bits of the tetrahedron's vertices 0..3 (nested: corner[p] is a subset of corner[q] for p < q)
};
// edge between tetrahedron vertices p < q: (edge id, vertex index within the object)
__device__ __forceinline__ void tet_edge(const TetCtx& c, int p, int q, long long& id, int& vid) {
    if (p > q) { const int x = p; p = q; q = x; }
    const unsigned u = c.v + corner_off(c.corner[p], c.n1, c.n2);
    const int d = kuhn_dir_of(c.corner[q] ^ c.corner[p]);
    id = 7ll * u + d;
    vid = edge_vertex_index(c.mask, c.escan, u, d);
}

__global__ void iso_emit_kernel(const float* __restrict__ grid, long long total, GridDims G, float level, snr_lattice lat,
                                const unsigned char* __restrict__ edge_mask, const int* __restrict__ edge_scan, const int* __restrict__ tri_scan,
                                const long long* __restrict__ vert_offset, const long long* __restrict__ tri_offset, float* __restrict__ verts,
                                int* __restrict__ faces) {
    const long long gid = grid_thread();
    if (gid >= total) return;
    const GridPoint p = grid_point(gid, G.nv, G.n1, G.n2);
    const long long b = p.b;
    const unsigned v = p.v;
    const float* f = grid + b * G.nv;
    const unsigned char* mask = edge_mask + b * G.nv;
    const int* escan = edge_scan + b * G.nv;

    // ---- the vertices of this grid vertex's crossing edges, in direction order
    const unsigned m = mask[v];
    if (m) {
        const float va = f[v];
        const int ia[3] = {p.i, p.j, p.k};
        long long w = vert_offset[b] + edge_vertex_index(mask, escan, v, 0);
        for (int d = 0; d < 7; ++d) {
            if (!((m >> d) & 1u)) continue;
            const int bits = kuhn_dir_bits(d);
            const float vb = f[v + corner_off(bits, G.n1, G.n2)];
            const float t = (level - va) / (vb - va);
            for (int a = 0; a < 3; ++a) verts[w * 3 + a] = lat.lo[a] + lat.h[a] * ((float)ia[a] + t * (float)((bits >> a) & 1));
            ++w;
        }
    }

    // ---- the triangles of the cell whose lower corner this is
    if (!corner_inside(G, p.i, p.j, p.k, 7)) return;
    const unsigned in = cell_inside_bits(f, v, G.n1, G.n2, level);
    if (in == 0 || in == 0xffu) return;
    long long w = tri_offset[b] + tri_scan[b * G.nc + cell_index(G, p.i, p.j, p.k)] - cell_tri_count(in);
    TetCtx c;
    c.mask = mask; c.escan = escan; c.v = v; c.n1 = G.n1; c.n2 = G.n2;
    for (int t = 0; t < 6; ++t) {
        c.corner[0] = 0;
        tet_corners(t, c.corner[1], c.corner[2]);
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

}  // namespace snr

using namespace snr;

extern "C" {

int snr_iso_count(const float* grid, int64_t n_grids, const snr_lattice* lattice, float level, uint8_t* tri_count, uint8_t* edge_mask,
                  uint8_t* edge_count, void* stream) {
    GridDims G;
    const int rc = grid_check(lattice, n_grids, 2, G);
    if (rc != SNR_OK) return rc;
    if (!grid || !tri_count || !edge_mask || !edge_count) return SNR_E_ARG;
    const long long total = n_grids * G.nv;
    if (total == 0) return SNR_OK;
    iso_count_kernel<<<grid_blocks(total), GRID_THREADS, 0, (hipStream_t)stream>>>(grid, total, G, level, tri_count, edge_mask, edge_count);
    return snr_check_launch_();
}

int snr_iso_emit(const float* grid, int64_t n_grids, const snr_lattice* lattice, float level, const uint8_t* edge_mask, const int32_t* edge_scan,
                 const int32_t* tri_scan, const int64_t* vert_offset, const int64_t* tri_offset, float* verts, int32_t* faces, void* stream) {
    GridDims G;
    const int rc = grid_check(lattice, n_grids, 2, G);
    if (rc != SNR_OK) return rc;
    if (!grid || !edge_mask || !edge_scan || !tri_scan || !vert_offset || !tri_offset) return SNR_E_ARG;
    const long long total = n_grids * G.nv;
    if (total == 0) return SNR_OK;
    // (verts / faces may be null when the scans say the surface is empty: nothing is then written)
    iso_emit_kernel<<<grid_blocks(total), GRID_THREADS, 0, (hipStream_t)stream>>>(grid, total, G, level, *lattice, edge_mask, edge_scan, tri_scan,
                                                                                   (const long long*)vert_offset, (const long long*)tri_offset, verts,
                                                                                   faces);
    return snr_check_launch_();
}

}  // extern "C"
