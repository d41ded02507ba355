// Mesh distance: the closest point of a packed triangle mesh to a query point, and area-uniform surface samples.
//
// The rules are the header's (include/supnerf_hip.h, "Mesh distance"); tests/nearest_restatement.py restates them in numpy.  In short:
// the answer of a query is the brute-force one -- over every face of its object the smallest float64 d^2 of Ericson's region walk, ties
// to the lowest face index -- and a uniform grid of cubic cells per object only decides how many faces are tested: a thread walks the
// cells around its query ring by ring and stops once no face it has not seen can still win.  Everything is float64 on the widened fp32
// inputs, one correctly rounded operation per written operation (no fma), so the kernel and the restatement give the same bits.
//
// One pass over faces counts the cells each one touches, a second writes the (cell, face) pairs behind the caller's scan; the caller
// sorts them and finds where each cell starts.  One thread per query, one per sample.  No atomics except the *bad flag; no launch reads
// what another thread of the same launch wrote.
#include "snr_nearest_grid.hpp"
#include "snr_host.hpp"

namespace snr {

constexpr double NEAREST_SLACK = 0x1p-40;              // D4's slack factor

// (D3 -- the grid of an object and the cell of a coordinate -- is snr_nearest_grid.hpp's)

// the index box of packed face f in its object's grid; false (and *bad) for a bad index, a non-finite vertex or an unusable grid
struct NearestBox {
    long long b, f_local, c0;
    int lo[3], hi[3], n[3];
};
__device__ __forceinline__ bool nearest_face_box(const float* __restrict__ verts, const int* __restrict__ faces,
                                                 const long long* __restrict__ voff, const long long* __restrict__ foff,
                                                 const float* __restrict__ cell, const float* __restrict__ grid_lo,
                                                 const float* __restrict__ grid_hi, const long long* __restrict__ cell_offset, long long B,
                                                 long long nV, long long n_cells, long long f, NearestBox& box) {
    const MeshFace m = mesh_face(faces, voff, foff, B, nV, f);
    if (!m.ok) return false;
    float mn[3], mx[3];
    bool finite = true;
    for (int a = 0; a < 3; ++a) {
        const float x0 = verts[(m.v0 + m.idx[0]) * 3 + a], x1 = verts[(m.v0 + m.idx[1]) * 3 + a], x2 = verts[(m.v0 + m.idx[2]) * 3 + a];
        finite = finite && nearest_finite(x0) && nearest_finite(x1) && nearest_finite(x2);
        mn[a] = fminf(fminf(x0, x1), x2);
        mx[a] = fmaxf(fmaxf(x0, x1), x2);
    }
    if (!finite) return false;
    const NearestGrid g = nearest_grid(cell, grid_lo, grid_hi, cell_offset, m.b, n_cells);
    if (!g.ok) return false;
    box.b = m.b;
    box.f_local = f - foff[m.b];
    box.c0 = g.c0;
    for (int a = 0; a < 3; ++a) {
        box.lo[a] = nearest_cell_of(g, a, (double)mn[a]);
        box.hi[a] = nearest_cell_of(g, a, (double)mx[a]);
        box.n[a] = g.n[a];
    }
    return true;
}

__global__ void nearest_count_kernel(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff,
                                     const long long* __restrict__ foff, const float* __restrict__ cell, const float* __restrict__ grid_lo,
                                     const float* __restrict__ grid_hi, const long long* __restrict__ cell_offset, long long B, long long nV,
                                     long long nF, long long n_cells, int* __restrict__ count, int* bad) {
    const long long f = grid_thread();
    if (f >= nF) return;
    NearestBox box;
    int c = 0;
    if (nearest_face_box(verts, faces, voff, foff, cell, grid_lo, grid_hi, cell_offset, B, nV, n_cells, f, box))
        c = (box.hi[0] - box.lo[0] + 1) * (box.hi[1] - box.lo[1] + 1) * (box.hi[2] - box.lo[2] + 1);          // (<= 2^24)
    else
        nearest_flag(bad);
    count[f] = c;
}

__global__ void nearest_emit_kernel(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff,
                                    const long long* __restrict__ foff, const float* __restrict__ cell, const float* __restrict__ grid_lo,
                                    const float* __restrict__ grid_hi, const long long* __restrict__ cell_offset,
                                    const long long* __restrict__ scan, long long B, long long nV, long long nF, long long n_cells,
                                    long long n_pairs, long long* __restrict__ pair_cell, int* __restrict__ pair_face) {
    const long long f = grid_thread();
    if (f >= nF) return;
    NearestBox box;
    if (!nearest_face_box(verts, faces, voff, foff, cell, grid_lo, grid_hi, cell_offset, B, nV, n_cells, f, box)) return;
    long long slot = scan[f];
    for (int x = box.lo[0]; x <= box.hi[0]; ++x)
        for (int y = box.lo[1]; y <= box.hi[1]; ++y)
            for (int z = box.lo[2]; z <= box.hi[2]; ++z, ++slot) {
                if (slot < 0 || slot >= n_pairs) continue;
                pair_cell[slot] = box.c0 + ((long long)x * box.n[1] + y) * box.n[2] + z;
                pair_face[slot] = (int)box.f_local;
            }
}

// ---- D1: point - triangle.  dot(x, y) = (x0 y0 + x1 y1) + x2 y2
__device__ __forceinline__ double nearest_dot(const double* x, const double* y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }

// the weights of the closest point of (a, b, c) to p and d^2; every operation as the header writes it
__device__ __forceinline__ double nearest_point_triangle(const double* p, const double* a, const double* b, const double* c, double* w) {
    double ab[3], ac[3], ap[3], bp[3], cp[3], e[3];
    for (int k = 0; k < 3; ++k) { ab[k] = b[k] - a[k]; ac[k] = c[k] - a[k]; ap[k] = p[k] - a[k]; }
    const double d1 = nearest_dot(ab, ap), d2 = nearest_dot(ac, ap);
    for (int k = 0; k < 3; ++k) bp[k] = p[k] - b[k];
    const double d3 = nearest_dot(ab, bp), d4 = nearest_dot(ac, bp);
    for (int k = 0; k < 3; ++k) cp[k] = p[k] - c[k];
    const double d5 = nearest_dot(ab, cp), d6 = nearest_dot(ac, cp);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const double e43 = d4 - d3, e56 = d5 - d6;
    if (d1 <= 0.0 && d2 <= 0.0) {                                            // vertex a
        w[0] = 1.0; w[1] = 0.0; w[2] = 0.0;
        for (int k = 0; k < 3; ++k) e[k] = ap[k];
    } else if (d3 >= 0.0 && d4 <= d3) {                                      // vertex b
        w[0] = 0.0; w[1] = 1.0; w[2] = 0.0;
        for (int k = 0; k < 3; ++k) e[k] = bp[k];
    } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0 && d1 - d3 > 0.0) {       // edge ab
        const double t = d1 / (d1 - d3);
        w[0] = 1.0 - t; w[1] = t; w[2] = 0.0;
        for (int k = 0; k < 3; ++k) e[k] = ap[k] - t * ab[k];
    } else if (d6 >= 0.0 && d5 <= d6) {                                      // vertex c
        w[0] = 0.0; w[1] = 0.0; w[2] = 1.0;
        for (int k = 0; k < 3; ++k) e[k] = cp[k];
    } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0 && d2 - d6 > 0.0) {       // edge ac
        const double t = d2 / (d2 - d6);
        w[0] = 1.0 - t; w[1] = 0.0; w[2] = t;
        for (int k = 0; k < 3; ++k) e[k] = ap[k] - t * ac[k];
    } else if (va <= 0.0 && e43 >= 0.0 && e56 >= 0.0 && e43 + e56 > 0.0) {   // edge bc
        const double t = e43 / (e43 + e56);
        w[0] = 0.0; w[1] = 1.0 - t; w[2] = t;
        for (int k = 0; k < 3; ++k) e[k] = bp[k] - t * (c[k] - b[k]);
    } else {                                                                 // interior
        const double s = (va + vb) + vc;
        const double v = vb / s, u = vc / s;
        w[0] = (1.0 - v) - u; w[1] = v; w[2] = u;
        for (int k = 0; k < 3; ++k) e[k] = (ap[k] - v * ab[k]) - u * ac[k];
    }
    return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
}

// ---- D2 and D4: one thread per query
struct NearestBest {
    double d2, w[3];
    int face;
};

__global__ void nearest_query_kernel(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff,
                                     const long long* __restrict__ foff, const float* __restrict__ points,
                                     const long long* __restrict__ qoff, const float* __restrict__ cell, const float* __restrict__ grid_lo,
                                     const float* __restrict__ grid_hi, const long long* __restrict__ cell_offset,
                                     const long long* __restrict__ cell_start, const int* __restrict__ pair_face, long long B, long long nV,
                                     long long nF, long long nQ, long long n_cells, long long n_pairs, int* __restrict__ out_face,
                                     float* __restrict__ out_w, double* __restrict__ out_d2, int* bad) {
    const long long q = grid_thread();
    if (q >= nQ) return;
    NearestBest best;
    best.d2 = __longlong_as_double(0x7ff0000000000000ll);                    // +inf
    best.face = -1;
    best.w[0] = best.w[1] = best.w[2] = 0.0;
    const long long b = mesh_entry_of(qoff, B, q);                           // the query's object, once
    const MeshObject o = mesh_object(voff, b, nV);
    const long long f0 = foff[b];
    long long F = foff[b + 1] - f0;
    if (f0 < 0 || F < 0 || f0 + F > nF) F = 0;
    const float pf[3] = {points[q * 3], points[q * 3 + 1], points[q * 3 + 2]};
    const bool finite = nearest_finite(pf[0]) && nearest_finite(pf[1]) && nearest_finite(pf[2]);
    if (finite && F > 0 && o.V > 0) {
        const NearestGrid g = nearest_grid(cell, grid_lo, grid_hi, cell_offset, b, n_cells);
        if (!g.ok) {
            nearest_flag(bad);
        } else {
            double p[3], tp[3];
            int c0[3];
            for (int a = 0; a < 3; ++a) {
                p[a] = (double)pf[a];
                tp[a] = p[a] - g.lo[a];
                c0[a] = nearest_cell_of(g, a, p[a]);
            }
            for (int r = 0; r < NEAREST_MAX_CELLS; ++r) {
                // the cells at Chebyshev distance r from c0 that lie inside the grid
                const int x0 = c0[0] - r > 0 ? c0[0] - r : 0, x1 = c0[0] + r < g.n[0] - 1 ? c0[0] + r : g.n[0] - 1;
                const int y0 = c0[1] - r > 0 ? c0[1] - r : 0, y1 = c0[1] + r < g.n[1] - 1 ? c0[1] + r : g.n[1] - 1;
                for (int x = x0; x <= x1; ++x)
                    for (int y = y0; y <= y1; ++y) {
                        const bool shell = x == c0[0] - r || x == c0[0] + r || y == c0[1] - r || y == c0[1] + r;
                        // on the shell in x or y every z of the block counts; inside it only the two caps
                        const int zstep = shell || r == 0 ? 1 : 2 * r;
                        for (int z = c0[2] - r; z <= c0[2] + r; z += zstep) {
                            if (z < 0 || z >= g.n[2]) continue;
                            const long long cid = g.c0 + ((long long)x * g.n[1] + y) * g.n[2] + z;
                            long long i = cell_start[cid];
                            const long long end = cell_start[cid + 1];
                            if (i < 0 || end > n_pairs) continue;
                            for (; i < end; ++i) {
                                const int fl = pair_face[i];
                                if (fl < 0 || (long long)fl >= F) continue;
                                const int ia = faces[(f0 + fl) * 3], ib = faces[(f0 + fl) * 3 + 1], ic = faces[(f0 + fl) * 3 + 2];
                                if (!(mesh_index_ok(ia, o.V) && mesh_index_ok(ib, o.V) && mesh_index_ok(ic, o.V))) {
                                    nearest_flag(bad);
                                    continue;
                                }
                                double va[3], vb[3], vc[3], w[3];
                                bool vfinite = true;
                                for (int k = 0; k < 3; ++k) {
                                    const float xa = verts[(o.v0 + ia) * 3 + k], xb = verts[(o.v0 + ib) * 3 + k], xc = verts[(o.v0 + ic) * 3 + k];
                                    vfinite = vfinite && nearest_finite(xa) && nearest_finite(xb) && nearest_finite(xc);
                                    va[k] = (double)xa; vb[k] = (double)xb; vc[k] = (double)xc;
                                }
                                if (!vfinite) continue;
                                const double d2 = nearest_point_triangle(p, va, vb, vc, w);
                                if (d2 < best.d2 || (d2 == best.d2 && fl < best.face)) {     // (false for a NaN)
                                    best.d2 = d2;
                                    best.face = fl;
                                    best.w[0] = w[0]; best.w[1] = w[1]; best.w[2] = w[2];
                                }
                            }
                        }
                    }
                // the nearest bounding plane of the block on a side where the grid goes on
                bool more = false;
                double m = 0.0;
                for (int a = 0; a < 3; ++a) {
                    const int kl = c0[a] - r, kh = c0[a] + r + 1;
                    if (kl >= 1) {
                        const double d = tp[a] - (double)kl * g.h;
                        m = !more || d < m ? d : m;
                        more = true;
                    }
                    if (kh <= g.n[a] - 1) {
                        const double d = (double)kh * g.h - tp[a];
                        m = !more || d < m ? d : m;
                        more = true;
                    }
                }
                if (!more) break;
                const double s = m - NEAREST_SLACK * (g.extent + m);
                if (s > 0.0 && s * s > best.d2) break;
            }
        }
    }
    out_face[q] = best.face;
    for (int k = 0; k < 3; ++k) out_w[q * 3 + k] = (float)best.w[k];
    out_d2[q] = best.d2;
}

// ---- D5: one thread per sample
__global__ void nearest_sample_kernel(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff,
                                      const long long* __restrict__ foff, const double* __restrict__ cum, const double* __restrict__ u,
                                      const long long* __restrict__ soff, long long B, long long nV, long long nF, long long nS,
                                      float* __restrict__ out_p, int* __restrict__ out_face, float* __restrict__ out_w, int* bad) {
    const long long s = grid_thread();
    if (s >= nS) return;
    const long long b = mesh_entry_of(soff, B, s);
    const long long i = s - soff[b], n = soff[b + 1] - soff[b];
    const MeshObject o = mesh_object(voff, b, nV);
    const long long f0 = foff[b];
    long long F = foff[b + 1] - f0;
    if (f0 < 0 || F < 0 || F > 0x7fffffffll || f0 + F > nF) F = 0;
    int face = -1;
    float w[3] = {0.f, 0.f, 0.f}, x[3] = {0.f, 0.f, 0.f};
    const double total = F > 0 ? cum[f0 + F - 1] : 0.0;
    if (total > 0.0 && total <= 1.7976931348623157e308 && n > 0) {
        const double u0 = u[s * 3], u1 = u[s * 3 + 1], u2 = u[s * 3 + 2];
        const double target = ((double)i + u0) / (double)n * total;
        // the first f with cum[f] > target; where rounding leaves none, the first f with cum[f] >= total: the last face with area
        const bool none = !(target < total);
        long long lo = 0, hi = F - 1;                                        // (cum[F - 1] = total passes either test)
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            const double c = cum[f0 + mid];
            if (none ? c >= total : c > target) hi = mid; else lo = mid + 1;
        }
        const int ia = faces[(f0 + lo) * 3], ib = faces[(f0 + lo) * 3 + 1], ic = faces[(f0 + lo) * 3 + 2];
        if (mesh_index_ok(ia, o.V) && mesh_index_ok(ib, o.V) && mesh_index_ok(ic, o.V)) {
            face = (int)lo;
            const double r = __dsqrt_rn(u1);
            const double w0 = 1.0 - r, w1 = r * (1.0 - u2), w2 = r * u2;
            for (int k = 0; k < 3; ++k) {
                const double a = (double)verts[(o.v0 + ia) * 3 + k], bb = (double)verts[(o.v0 + ib) * 3 + k], c = (double)verts[(o.v0 + ic) * 3 + k];
                x[k] = (float)((w0 * a + w1 * bb) + w2 * c);
            }
            w[0] = (float)w0; w[1] = (float)w1; w[2] = (float)w2;
        } else {
            nearest_flag(bad);
        }
    }
    out_face[s] = face;
    for (int k = 0; k < 3; ++k) { out_p[s * 3 + k] = x[k]; out_w[s * 3 + k] = w[k]; }
}

}  // namespace snr

using namespace snr;

extern "C" {

int snr_nearest_count(const float* verts, const int32_t* faces, const int64_t* vert_offset, const int64_t* face_offset, const float* cell,
                      const float* grid_lo, const float* grid_hi, const int64_t* cell_offset, int64_t n_objects, int64_t n_verts,
                      int64_t n_faces, int64_t n_cells, int32_t* count, int32_t* bad, void* stream) {
    int rc = packed_sizes(n_objects, n_verts, n_faces);
    if (rc != SNR_OK) return rc;
    rc = packed_sizes(0, n_cells, 0);
    if (rc != SNR_OK) return rc;
    if (!bad) return SNR_E_ARG;
    if (n_faces == 0) return SNR_OK;
    if (n_objects == 0 || !verts || !faces || !vert_offset || !face_offset || !cell || !grid_lo || !grid_hi || !cell_offset || !count)
        return SNR_E_ARG;
    nearest_count_kernel<<<grid_blocks(n_faces), GRID_THREADS, 0, (hipStream_t)stream>>>(
        verts, faces, (const long long*)vert_offset, (const long long*)face_offset, cell, grid_lo, grid_hi, (const long long*)cell_offset,
        n_objects, n_verts, n_faces, n_cells, count, bad);
    return snr_check_launch_();
}

int snr_nearest_emit(const float* verts, const int32_t* faces, const int64_t* vert_offset, const int64_t* face_offset, const float* cell,
                     const float* grid_lo, const float* grid_hi, const int64_t* cell_offset, const int64_t* count_scan, int64_t n_objects,
                     int64_t n_verts, int64_t n_faces, int64_t n_cells, int64_t n_pairs, int64_t* pair_cell, int32_t* pair_face,
                     void* stream) {
    int rc = packed_sizes(n_objects, n_verts, n_faces);
    if (rc != SNR_OK) return rc;
    rc = packed_sizes(0, n_cells, n_pairs);
    if (rc != SNR_OK) return rc;
    if (n_faces == 0 || n_pairs == 0) return SNR_OK;
    if (n_objects == 0 || !verts || !faces || !vert_offset || !face_offset || !cell || !grid_lo || !grid_hi || !cell_offset ||
        !count_scan || !pair_cell || !pair_face)
        return SNR_E_ARG;
    nearest_emit_kernel<<<grid_blocks(n_faces), GRID_THREADS, 0, (hipStream_t)stream>>>(
        verts, faces, (const long long*)vert_offset, (const long long*)face_offset, cell, grid_lo, grid_hi, (const long long*)cell_offset,
        (const long long*)count_scan, n_objects, n_verts, n_faces, n_cells, n_pairs, (long long*)pair_cell, pair_face);
    return snr_check_launch_();
}

int snr_nearest_query(const float* verts, const int32_t* faces, const int64_t* vert_offset, const int64_t* face_offset, const float* points,
                      const int64_t* query_offset, const float* cell, const float* grid_lo, const float* grid_hi, const int64_t* cell_offset,
                      const int64_t* cell_start, const int32_t* pair_face, int64_t n_objects, int64_t n_verts, int64_t n_faces,
                      int64_t n_queries, int64_t n_cells, int64_t n_pairs, int32_t* face, float* weights, double* dist2, int32_t* bad,
                      void* stream) {
    int rc = packed_sizes(n_objects, n_verts, n_faces);
    if (rc != SNR_OK) return rc;
    rc = packed_sizes(0, n_queries, 0);
    if (rc != SNR_OK) return rc;
    rc = packed_sizes(0, n_cells, n_pairs);
    if (rc != SNR_OK) return rc;
    if (!bad) return SNR_E_ARG;
    if (n_queries == 0) return SNR_OK;
    if (n_objects == 0 || !vert_offset || !face_offset || !points || !query_offset || !cell || !grid_lo || !grid_hi || !cell_offset ||
        !cell_start || !face || !weights || !dist2)
        return SNR_E_ARG;
    if ((n_faces && (!faces || !verts)) || (n_pairs && !pair_face)) return SNR_E_ARG;
    nearest_query_kernel<<<grid_blocks(n_queries), GRID_THREADS, 0, (hipStream_t)stream>>>(
        verts, faces, (const long long*)vert_offset, (const long long*)face_offset, points, (const long long*)query_offset, cell, grid_lo,
        grid_hi, (const long long*)cell_offset, (const long long*)cell_start, pair_face, n_objects, n_verts, n_faces, n_queries, n_cells,
        n_pairs, face, weights, dist2, bad);
    return snr_check_launch_();
}

int snr_surface_sample(const float* verts, const int32_t* faces, const int64_t* vert_offset, const int64_t* face_offset, const double* cum_area,
                       const double* uniforms, const int64_t* sample_offset, int64_t n_objects, int64_t n_verts, int64_t n_faces,
                       int64_t n_samples, float* points, int32_t* face, float* weights, int32_t* bad, void* stream) {
    int rc = packed_sizes(n_objects, n_verts, n_faces);
    if (rc != SNR_OK) return rc;
    rc = packed_sizes(0, n_samples, 0);
    if (rc != SNR_OK) return rc;
    if (!bad) return SNR_E_ARG;
    if (n_samples == 0) return SNR_OK;
    if (n_objects == 0 || !vert_offset || !face_offset || !uniforms || !sample_offset || !points || !face || !weights) return SNR_E_ARG;
    if (n_faces && (!faces || !verts || !cum_area)) return SNR_E_ARG;
    nearest_sample_kernel<<<grid_blocks(n_samples), GRID_THREADS, 0, (hipStream_t)stream>>>(
        verts, faces, (const long long*)vert_offset, (const long long*)face_offset, cum_area, uniforms, (const long long*)sample_offset,
        n_objects, n_verts, n_faces, n_samples, points, face, weights, bad);
    return snr_check_launch_();
}

}  // extern "C"
