// Mesh containment: the integer winding number along +z of a packed triangle mesh at query points and on lattices.
//
// The rules are the header's (include/supnerf_hip.h, "Mesh containment", W1 - W6); tests/inside_restatement.py restates them in numpy.  In
// short: the answer of a query is the brute-force one -- over every face of its object the signed count of the faces the ray from p in
// direction +z crosses, with a half-open box guard (W1), an edge-side rule that gives both faces of an edge the same bits and a point under
// an edge or a vertex to exactly one face (W2, W3), and a division-free test that the face is ahead (W4) -- and the grid of "Mesh distance"
// D3 only decides how many faces are tested: a thread walks the z-column of cells above its query, and a face listed in several cells of
// that column counts in one of them (W5).  Everything is float64 on the widened fp32 inputs, one rounded operation per written operation
// (no fma); the results are integers and the kernels give the restatement's.
//
// One thread per query.  On a lattice (W6) one thread per tile of INSIDE_TILE consecutive z-points of one (object, i, j) column: whatever
// does not depend on p_z -- the guard in x and y, the three edge sides, the normal and the bracket of W4 -- is done once per face and
// tile, and per z-point a compare, a subtraction, a multiply-add and a compare remain.  No atomics except the *bad flag; no launch reads
// what another thread of the same launch wrote.
#include "snr_nearest_grid.hpp"
#include "snr_host.hpp"

namespace snr {

constexpr int INSIDE_TILE = 16;                        // z-points of a lattice column per thread (W6)

__device__ __forceinline__ int inside_sign(double x) { return (int)(x > 0.0) - (int)(x < 0.0); }

// ---- W2: the side of p of the directed edge u -> v, from the endpoints in lexicographic (x, y) order
__device__ __forceinline__ int inside_edge(double ux, double uy, double vx, double vy, double px, double py) {
    const bool swapped = vx < ux || (vx == ux && vy < uy);
    const double ax = swapped ? vx : ux, ay = swapped ? vy : uy, bx = swapped ? ux : vx, by = swapped ? uy : vy;
    const double dx = bx - ax, dy = by - ay;
    const double e = dx * (py - ay) - dy * (px - ax);
    int s = inside_sign(e);
    if (s == 0) s = inside_sign(-dy);
    if (s == 0) s = inside_sign(dx);
    return swapped ? -s : s;
}

// the object of a query or a column: its vertices, its faces and its grid
struct InsideObject {
    MeshObject o;
    long long f0, F;
    NearestGrid g;
    bool live;                   // it has vertices, faces and a usable grid
};
__device__ __forceinline__ InsideObject inside_object(const long long* __restrict__ voff, const long long* __restrict__ foff,
                                                      const float* __restrict__ cell, const float* __restrict__ grid_lo,
                                                      const float* __restrict__ grid_hi, const long long* __restrict__ cell_offset,
                                                      long long b, long long nV, long long nF, long long n_cells, int* bad) {
    InsideObject s;
    s.o = mesh_object(voff, b, nV);
    s.f0 = foff[b];
    s.F = foff[b + 1] - s.f0;
    if (s.f0 < 0 || s.F < 0 || s.f0 + s.F > nF) s.F = 0;
    s.live = s.F > 0 && s.o.V > 0;
    s.g.ok = false;
    if (s.live) {
        s.g = nearest_grid(cell, grid_lo, grid_hi, cell_offset, b, n_cells);
        if (!s.g.ok) nearest_flag(bad);
        s.live = s.g.ok;
    }
    return s;
}

// what a face that can count for (p_x, p_y) keeps for the z-points above or below it
struct InsideFace {
    int sigma;                   // W3
    float zmax;                  // W1's bound on p_z
    double bracket, nz, az;      // W4: t = bracket + nz (az - p_z)
};

// Listed face i of cell k of the column of (px, py), walked from cell k_first on: false unless W1 (in x and y), W3 and the once-only
// rule of W5 let it count for some p_z.  Every index is range-checked before it is used; a bad index sets *bad.
__device__ __forceinline__ bool inside_face(const float* __restrict__ verts, const int* __restrict__ faces, const int* __restrict__ pair_face,
                                            const InsideObject& s, long long i, int k, int k_first, float px, float py, InsideFace& r,
                                            int* bad) {
    const int fl = pair_face[i];
    if (fl < 0 || (long long)fl >= s.F) return false;
    const int ia = faces[(s.f0 + fl) * 3], ib = faces[(s.f0 + fl) * 3 + 1], ic = faces[(s.f0 + fl) * 3 + 2];
    if (!(mesh_index_ok(ia, s.o.V) && mesh_index_ok(ib, s.o.V) && mesh_index_ok(ic, s.o.V))) {
        nearest_flag(bad);
        return false;
    }
    float a[3], b[3], c[3];
    bool finite = true;
    for (int d = 0; d < 3; ++d) {
        a[d] = verts[(s.o.v0 + ia) * 3 + d]; b[d] = verts[(s.o.v0 + ib) * 3 + d]; c[d] = verts[(s.o.v0 + ic) * 3 + d];
        finite = finite && nearest_finite(a[d]) && nearest_finite(b[d]) && nearest_finite(c[d]);
    }
    if (!finite) return false;
    // W1 in x and y
    if (!(fminf(fminf(a[0], b[0]), c[0]) <= px && px < fmaxf(fmaxf(a[0], b[0]), c[0]))) return false;
    if (!(fminf(fminf(a[1], b[1]), c[1]) <= py && py < fmaxf(fmaxf(a[1], b[1]), c[1]))) return false;
    // W5: of the cells of this column that list the face, the one where it counts
    const int kf = nearest_cell_of(s.g, 2, (double)fminf(fminf(a[2], b[2]), c[2]));
    if ((kf > k_first ? kf : k_first) != k) return false;
    // W2, W3
    const double ax = (double)a[0], ay = (double)a[1], az = (double)a[2], bx = (double)b[0], by = (double)b[1], bz = (double)b[2];
    const double cx = (double)c[0], cy = (double)c[1], cz = (double)c[2], qx = (double)px, qy = (double)py;
    const int s0 = inside_edge(ax, ay, bx, by, qx, qy);
    if (s0 == 0 || inside_edge(bx, by, cx, cy, qx, qy) != s0 || inside_edge(cx, cy, ax, ay, qx, qy) != s0) return false;
    // W4
    const double x1 = bx - ax, y1 = by - ay, z1 = bz - az, x2 = cx - ax, y2 = cy - ay, z2 = cz - az;
    const double nx = y1 * z2 - z1 * y2, ny = z1 * x2 - x1 * z2;
    r.nz = x1 * y2 - y1 * x2;
    r.bracket = nx * (ax - qx) + ny * (ay - qy);
    r.az = az;
    r.sigma = s0;
    r.zmax = fmaxf(fmaxf(a[2], b[2]), c[2]);
    return true;
}

// the contribution of a kept face to the point at height pz (finite)
__device__ __forceinline__ int inside_term(const InsideFace& r, float pz) {
    if (!(pz < r.zmax)) return 0;
    const double t = r.bracket + r.nz * (r.az - (double)pz);
    return (r.sigma > 0 ? t > 0.0 : t < 0.0) ? r.sigma : 0;
}

// ---- W1 - W5: one thread per query
__global__ void __launch_bounds__(GRID_THREADS) inside_query_kernel(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff,
                                    const long long* __restrict__ foff, const float* __restrict__ points, const long long* __restrict__ qoff,
                                    const float* __restrict__ cell, const float* __restrict__ grid_lo, const float* __restrict__ grid_hi,
                                    const long long* __restrict__ cell_offset, const long long* __restrict__ cell_start,
                                    const int* __restrict__ pair_face, long long B, long long nV, long long nF, long long nQ,
                                    long long n_cells, long long n_pairs, int* __restrict__ winding, int* bad) {
    const long long q = grid_thread();
    if (q >= nQ) return;
    int w = 0;
    const float px = points[q * 3], py = points[q * 3 + 1], pz = points[q * 3 + 2];
    if (nearest_finite(px) && nearest_finite(py) && nearest_finite(pz)) {
        const long long b = mesh_entry_of(qoff, B, q);                       // the query's object, once
        const InsideObject s = inside_object(voff, foff, cell, grid_lo, grid_hi, cell_offset, b, nV, nF, n_cells, bad);
        if (s.live) {
            const int cx = nearest_cell_of(s.g, 0, (double)px), cy = nearest_cell_of(s.g, 1, (double)py);
            const int k_first = nearest_cell_of(s.g, 2, (double)pz);
            const long long column = s.g.c0 + ((long long)cx * s.g.n[1] + cy) * s.g.n[2];
            for (int k = k_first; k < s.g.n[2]; ++k) {
                long long i = cell_start[column + k];
                const long long end = cell_start[column + k + 1];
                if (i < 0 || end > n_pairs) continue;
                for (; i < end; ++i) {
                    InsideFace r;
                    if (inside_face(verts, faces, pair_face, s, i, k, k_first, px, py, r, bad)) w += inside_term(r, pz);
                }
            }
        }
    }
    winding[q] = w;
}

// ---- W6: one thread per INSIDE_TILE z-points of one (object, i, j) column
__global__ void __launch_bounds__(GRID_THREADS) inside_lattice_kernel(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff,
                                      const long long* __restrict__ foff, const float* __restrict__ cell, const float* __restrict__ grid_lo,
                                      const float* __restrict__ grid_hi, const long long* __restrict__ cell_offset,
                                      const long long* __restrict__ cell_start, const int* __restrict__ pair_face,
                                      const float* __restrict__ lat_lo, const float* __restrict__ lat_h, long long B, long long nV,
                                      long long nF, long long n_cells, long long n_pairs, long long n1, long long n2, long long tiles,
                                      long long per_obj, long long n_threads, int* __restrict__ winding, int* bad) {
    const long long gid = grid_thread();
    if (gid >= n_threads) return;
    long long rest;
    const long long b = grid_object(gid, per_obj, rest);
    const long long col = rest / tiles, tile = rest - col * tiles;
    const long long i = col / n1, j = col - i * n1;
    const long long z0 = tile * INSIDE_TILE;
    const int count = n2 - z0 < INSIDE_TILE ? (int)(n2 - z0) : INSIDE_TILE;              // z-points of this tile
    const float px = lat_lo[b * 3] + lat_h[b * 3] * (float)i, py = lat_lo[b * 3 + 1] + lat_h[b * 3 + 1] * (float)j;
    const float zl = lat_lo[b * 3 + 2], zh = lat_h[b * 3 + 2];
    int w[INSIDE_TILE];
    float lowest = 0.f;
    bool any = false;                                                        // a z-point of the tile that is finite
#pragma unroll
    for (int t = 0; t < INSIDE_TILE; ++t) {
        w[t] = 0;
        const float pz = zl + zh * (float)(z0 + t);
        if (t < count && nearest_finite(pz)) {
            lowest = !any || pz < lowest ? pz : lowest;
            any = true;
        }
    }
    if (any && nearest_finite(px) && nearest_finite(py)) {
        const InsideObject s = inside_object(voff, foff, cell, grid_lo, grid_hi, cell_offset, b, nV, nF, n_cells, bad);
        if (s.live) {
            const int cx = nearest_cell_of(s.g, 0, (double)px), cy = nearest_cell_of(s.g, 1, (double)py);
            const int k_first = nearest_cell_of(s.g, 2, (double)lowest);     // the cell of the tile's lowest point: W5 from there on
            const long long column = s.g.c0 + ((long long)cx * s.g.n[1] + cy) * s.g.n[2];
            for (int k = k_first; k < s.g.n[2]; ++k) {
                long long e = cell_start[column + k];
                const long long end = cell_start[column + k + 1];
                if (e < 0 || end > n_pairs) continue;
                for (; e < end; ++e) {
                    InsideFace r;
                    if (!inside_face(verts, faces, pair_face, s, e, k, k_first, px, py, r, bad)) continue;
#pragma unroll
                    for (int t = 0; t < INSIDE_TILE; ++t) {
                        const float pz = zl + zh * (float)(z0 + t);          // (formed again: cheaper than keeping the tile's heights)
                        if (t < count && nearest_finite(pz)) w[t] += inside_term(r, pz);
                    }
                }
            }
        }
    }
    int* out = winding + (b * (per_obj / tiles) + col) * n2 + z0;
#pragma unroll
    for (int t = 0; t < INSIDE_TILE; ++t)
        if (t < count) out[t] = w[t];
}

// the pointers both entry points take for the mesh and its grid
inline int inside_mesh_args(const float* verts, const int32_t* faces, const int64_t* vert_offset, const int64_t* face_offset, const float* cell,
                            const float* grid_lo, const float* grid_hi, const int64_t* cell_offset, const int64_t* cell_start,
                            const int32_t* pair_face, int64_t n_objects, int64_t n_faces, int64_t n_pairs) {
    if (n_objects == 0 || !vert_offset || !face_offset || !cell || !grid_lo || !grid_hi || !cell_offset || !cell_start) return SNR_E_ARG;
    if ((n_faces && (!faces || !verts)) || (n_pairs && !pair_face)) return SNR_E_ARG;
    return SNR_OK;
}

}  // namespace snr

using namespace snr;

extern "C" {

int snr_inside_query(const float* verts, const int32_t* faces, const int64_t* vert_offset, const int64_t* face_offset, const float* points,
                     const int64_t* query_offset, const float* cell, const float* grid_lo, const float* grid_hi, const int64_t* cell_offset,
                     const int64_t* cell_start, const int32_t* pair_face, int64_t n_objects, int64_t n_verts, int64_t n_faces,
                     int64_t n_queries, int64_t n_cells, int64_t n_pairs, int32_t* winding, int32_t* bad, void* stream) {
    int rc = packed_sizes(n_objects, n_verts, n_faces);
    if (rc != SNR_OK) return rc;
    rc = packed_sizes(0, n_queries, 0);
    if (rc != SNR_OK) return rc;
    rc = packed_sizes(0, n_cells, n_pairs);
    if (rc != SNR_OK) return rc;
    if (!bad) return SNR_E_ARG;
    if (n_queries == 0) return SNR_OK;
    rc = inside_mesh_args(verts, faces, vert_offset, face_offset, cell, grid_lo, grid_hi, cell_offset, cell_start, pair_face, n_objects,
                          n_faces, n_pairs);
    if (rc != SNR_OK) return rc;
    if (!points || !query_offset || !winding) return SNR_E_ARG;
    inside_query_kernel<<<grid_blocks(n_queries), GRID_THREADS, 0, (hipStream_t)stream>>>(
        verts, faces, (const long long*)vert_offset, (const long long*)face_offset, points, (const long long*)query_offset, cell, grid_lo,
        grid_hi, (const long long*)cell_offset, (const long long*)cell_start, pair_face, n_objects, n_verts, n_faces, n_queries, n_cells,
        n_pairs, winding, bad);
    return snr_check_launch_();
}

int snr_inside_lattice(const float* verts, const int32_t* faces, const int64_t* vert_offset, const int64_t* face_offset, const float* cell,
                       const float* grid_lo, const float* grid_hi, const int64_t* cell_offset, const int64_t* cell_start,
                       const int32_t* pair_face, const float* lat_lo, const float* lat_h, int64_t n_objects, int64_t n_verts, int64_t n_faces,
                       int64_t n_cells, int64_t n_pairs, int64_t n_x, int64_t n_y, int64_t n_z, int32_t* winding, int32_t* bad, void* stream) {
    int rc = packed_sizes(n_objects, n_verts, n_faces);
    if (rc != SNR_OK) return rc;
    rc = packed_sizes(0, n_cells, n_pairs);
    if (rc != SNR_OK) return rc;
    rc = packed_sizes(0, n_x, n_y);
    if (rc != SNR_OK) return rc;
    rc = packed_sizes(0, n_z, 0);
    if (rc != SNR_OK) return rc;
    if (!bad) return SNR_E_ARG;
    if (n_objects == 0 || n_x == 0 || n_y == 0 || n_z == 0) return SNR_OK;
    // the lattice points of the launch, without overflow: each factor is at most 2^38 here
    if (n_x > PACKED_MAX_ITEMS / n_y) return SNR_E_UNSUPPORTED;
    const long long columns = (long long)n_x * n_y;
    if (columns > PACKED_MAX_ITEMS / n_z) return SNR_E_UNSUPPORTED;
    if (columns * n_z > PACKED_MAX_ITEMS / n_objects) return SNR_E_UNSUPPORTED;
    rc = inside_mesh_args(verts, faces, vert_offset, face_offset, cell, grid_lo, grid_hi, cell_offset, cell_start, pair_face, n_objects,
                          n_faces, n_pairs);
    if (rc != SNR_OK) return rc;
    if (!lat_lo || !lat_h || !winding) return SNR_E_ARG;
    const long long tiles = ((long long)n_z + INSIDE_TILE - 1) / INSIDE_TILE;
    const long long per_obj = columns * tiles, n_threads = per_obj * n_objects;          // (<= the lattice points: <= 2^38)
    inside_lattice_kernel<<<grid_blocks(n_threads), GRID_THREADS, 0, (hipStream_t)stream>>>(
        verts, faces, (const long long*)vert_offset, (const long long*)face_offset, cell, grid_lo, grid_hi, (const long long*)cell_offset,
        (const long long*)cell_start, pair_face, lat_lo, lat_h, n_objects, n_verts, n_faces, n_cells, n_pairs, n_y, n_z, tiles, per_obj,
        n_threads, winding, bad);
    return snr_check_launch_();
}

}  // extern "C"
