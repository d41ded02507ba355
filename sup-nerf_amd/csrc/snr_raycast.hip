// Mesh ray casting: the first face of a packed triangle mesh that a ray hits, and the signed and total number of faces it crosses.
//
// The rules are the header's (include/supnerf_hip.h, "Mesh ray casting", R1 - R6); tests/raycast_restatement.py restates them in numpy.  In
// short: the answer of a ray is the brute-force one over every face of its object -- the ray's own sheared frame (R1), an edge-side rule
// that gives both faces of an edge the same bits and a ray through an edge or a vertex to exactly one face (R2, R3), the depth from the
// three edge values with one divide (R4), the smallest depth with ties to the lowest face (R5) -- and the grid of "Mesh distance" D3 only
// decides how many faces are tested: a thread clips its ray against the object's bounds and walks the slabs of cells along the ray's
// dominant axis, in each the small rectangle of cells the ray can touch (R6).  Everything is float64 on the widened fp32 inputs, one
// rounded operation per written operation (no fma).
//
// One thread per ray; the frame of R1 stays in registers across the walk.  The per-face test has no divide until the face has passed R3.
// No atomics except the *bad flag; no launch reads what another thread of the same launch wrote.
#include "snr_nearest_grid.hpp"
#include "snr_host.hpp"

namespace snr {

constexpr double RAYCAST_SLACK = 0x1p-40;              // R6

__device__ __forceinline__ int raycast_sign(double x) { return (int)(x > 0.0) - (int)(x < 0.0); }
template <typename T>
__device__ __forceinline__ T raycast_pick(const T (&x)[3], int k) { return k == 0 ? x[0] : (k == 1 ? x[1] : x[2]); }
__device__ __forceinline__ int raycast_clamp(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

// ---- R2: the side of the origin of the directed edge u -> v and the edge's value e, from the endpoints in lexicographic (x', y') order
__device__ __forceinline__ int raycast_edge(double ux, double uy, double vx, double vy, double& e) {
    const bool swapped = vx < ux || (vx == ux && vy < uy);
    const double ax = swapped ? vx : ux, ay = swapped ? vy : uy, bx = swapped ? ux : vx, by = swapped ? uy : vy;
    const double dx = bx - ax, dy = by - ay;
    const double c = dy * ax - dx * ay;
    int s = raycast_sign(c);
    if (s == 0) s = raycast_sign(-dy);
    if (s == 0) s = raycast_sign(dx);
    e = swapped ? -c : c;
    return swapped ? -s : s;
}

// the object of a ray: its vertices, its faces and its grid
struct RaycastObject {
    MeshObject o;
    long long f0, F;
    NearestGrid g;
    double hi[3];                // grid_hi, widened
    bool live;                   // it has vertices, faces and a usable grid
};
__device__ __forceinline__ RaycastObject raycast_object(const long long* __restrict__ voff, const long long* __restrict__ foff,
                                                        const float* __restrict__ cell, const float* __restrict__ grid_lo,
                                                        const float* __restrict__ grid_hi, const long long* __restrict__ cell_offset,
                                                        long long b, long long nV, long long nF, long long n_cells, int* bad) {
    RaycastObject s;
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
        for (int a = 0; a < 3; ++a) s.hi[a] = (double)grid_hi[b * 3 + a];
    }
    return s;
}

// ---- R1: the frame of a ray
struct RaycastRay {
    double o[3], d[3];           // origin and direction, widened
    double ox, oy, oz;           // o[kx], o[ky], o[kz]
    double Sx, Sy, Sz, tmin, tmax;
    int kx, ky, kz;
};
__device__ __forceinline__ void raycast_frame(RaycastRay& r) {
    const double a0 = fabs(r.d[0]), a1 = fabs(r.d[1]), a2 = fabs(r.d[2]);
    r.kz = a0 >= a1 ? (a0 >= a2 ? 0 : 2) : (a1 >= a2 ? 1 : 2);               // (ties to the lowest axis)
    r.kx = r.kz == 2 ? 0 : r.kz + 1;
    r.ky = r.kx == 2 ? 0 : r.kx + 1;
    const double dz = raycast_pick(r.d, r.kz);
    if (dz < 0.0) { const int k = r.kx; r.kx = r.ky; r.ky = k; }
    r.Sx = raycast_pick(r.d, r.kx) / dz;
    r.Sy = raycast_pick(r.d, r.ky) / dz;
    r.Sz = 1.0 / dz;
    r.ox = raycast_pick(r.o, r.kx); r.oy = raycast_pick(r.o, r.ky); r.oz = raycast_pick(r.o, r.kz);
}

// what a face that counts leaves behind
struct RaycastTerm {
    double U, V, W, det, t;
    int sigma;                   // R3: +1 the ray leaves through the face (d . n > 0), -1 it enters
};

// Listed face fl of object s against ray r by R1 - R4: false unless it counts.  lo, hi: the extremes of its corners along (kx, ky, kz), for
// the caller's cell rule.  Every index is range-checked before it is used; a bad index sets *bad.
__device__ __forceinline__ bool raycast_face(const float* __restrict__ verts, const int* __restrict__ faces, const RaycastObject& s, int fl,
                                             const RaycastRay& r, RaycastTerm& h, double (&lo)[3], double (&hi)[3], int* bad) {
    if (fl < 0 || (long long)fl >= s.F) return false;
    const int ia = faces[(s.f0 + fl) * 3], ib = faces[(s.f0 + fl) * 3 + 1], ic = faces[(s.f0 + fl) * 3 + 2];
    if (!(mesh_index_ok(ia, s.o.V) && mesh_index_ok(ib, s.o.V) && mesh_index_ok(ic, s.o.V))) {
        nearest_flag(bad);
        return false;
    }
    double a[3], b[3], c[3];
    bool finite = true;
    for (int k = 0; k < 3; ++k) {
        const float fa = verts[(s.o.v0 + ia) * 3 + k], fb = verts[(s.o.v0 + ib) * 3 + k], fc = verts[(s.o.v0 + ic) * 3 + k];
        finite = finite && nearest_finite(fa) && nearest_finite(fb) && nearest_finite(fc);
        a[k] = (double)fa; b[k] = (double)fb; c[k] = (double)fc;
    }
    if (!finite) return false;
    // the corners in the frame's axis order (kx, ky, kz), and their extremes for the caller's cell rule
    const double pa[3] = {raycast_pick(a, r.kx), raycast_pick(a, r.ky), raycast_pick(a, r.kz)};
    const double pb[3] = {raycast_pick(b, r.kx), raycast_pick(b, r.ky), raycast_pick(b, r.kz)};
    const double pc[3] = {raycast_pick(c, r.kx), raycast_pick(c, r.ky), raycast_pick(c, r.kz)};
    for (int k = 0; k < 3; ++k) {
        lo[k] = fmin(fmin(pa[k], pb[k]), pc[k]);
        hi[k] = fmax(fmax(pa[k], pb[k]), pc[k]);
    }
    // R1
    const double az = pa[2] - r.oz, bz = pb[2] - r.oz, cz = pc[2] - r.oz;
    const double xa = (pa[0] - r.ox) - r.Sx * az, ya = (pa[1] - r.oy) - r.Sy * az;
    const double xb = (pb[0] - r.ox) - r.Sx * bz, yb = (pb[1] - r.oy) - r.Sy * bz;
    const double xc = (pc[0] - r.ox) - r.Sx * cz, yc = (pc[1] - r.oy) - r.Sy * cz;
    // R2, R3
    const int s0 = raycast_edge(xa, ya, xb, yb, h.W);
    if (s0 == 0 || raycast_edge(xb, yb, xc, yc, h.U) != s0 || raycast_edge(xc, yc, xa, ya, h.V) != s0) return false;
    // R4: the one divide
    h.sigma = s0;
    h.det = (h.U + h.V) + h.W;
    h.t = ((h.U * (r.Sz * az) + h.V * (r.Sz * bz)) + h.W * (r.Sz * cz)) / h.det;
    return r.tmin < h.t && h.t < r.tmax;
}

// ---- R1 - R6: one thread per ray.  FIRST: the first hit; else the crossings
template <bool FIRST>
__global__ void __launch_bounds__(GRID_THREADS) raycast_kernel(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff,
                               const long long* __restrict__ foff, const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                               const long long* __restrict__ roff, const float* __restrict__ t_min, const float* __restrict__ t_max, int cull,
                               const float* __restrict__ cell, const float* __restrict__ grid_lo, const float* __restrict__ grid_hi,
                               const long long* __restrict__ cell_offset, const long long* __restrict__ cell_start,
                               const int* __restrict__ pair_face, long long B, long long nV, long long nF, long long nR, long long n_cells,
                               long long n_pairs, int* __restrict__ out_face, double* __restrict__ out_t, float* __restrict__ out_w,
                               signed char* __restrict__ out_side, int* __restrict__ out_signed, int* __restrict__ out_total, int* bad) {
    const long long q = grid_thread();
    if (q >= nR) return;
    RaycastTerm best;
    best.U = best.V = best.W = 0.0; best.det = 1.0; best.sigma = 0;
    best.t = __longlong_as_double(0x7ff0000000000000ll);                     // +inf
    int best_face = -1, n_signed = 0, n_total = 0;
    RaycastRay r;
    bool finite = true;
    for (int a = 0; a < 3; ++a) {
        const float fo = rays_o[q * 3 + a], fd = rays_d[q * 3 + a];
        finite = finite && nearest_finite(fo) && nearest_finite(fd);
        r.o[a] = (double)fo; r.d[a] = (double)fd;
    }
    r.tmin = (double)t_min[q]; r.tmax = (double)t_max[q];
    if (finite && (r.d[0] != 0.0 || r.d[1] != 0.0 || r.d[2] != 0.0) && r.tmin < r.tmax) {
        const long long b = mesh_entry_of(roff, B, q);                       // the ray's object, once
        const RaycastObject s = raycast_object(voff, foff, cell, grid_lo, grid_hi, cell_offset, b, nV, nF, n_cells, bad);
        if (s.live) {
            raycast_frame(r);
            // R6: clip against the bounds widened by the slack
            double m = 0.0;
            for (int a = 0; a < 3; ++a) m = fmax(m, fmax(s.g.lo[a] - r.o[a], r.o[a] - s.hi[a]));
            const double slack = RAYCAST_SLACK * (s.g.extent + m);
            double ta = r.tmin, tb = r.tmax;
            bool in = true;
            for (int a = 0; a < 3; ++a) {
                if (r.d[a] != 0.0) {
                    const double t1 = ((s.g.lo[a] - slack) - r.o[a]) / r.d[a], t2 = ((s.hi[a] + slack) - r.o[a]) / r.d[a];
                    ta = fmax(ta, fmin(t1, t2));
                    tb = fmin(tb, fmax(t1, t2));
                } else if (r.o[a] < s.g.lo[a] - slack || r.o[a] > s.hi[a] + slack) {
                    in = false;
                }
            }
            if (in && ta <= tb) {
                const double dz = raycast_pick(r.d, r.kz), dx = raycast_pick(r.d, r.kx), dy = raycast_pick(r.d, r.ky);
                // the grid with its axes in the frame's order (kx, ky, kz): every cell lookup below names a constant axis
                NearestGrid g = s.g;
                g.lo[0] = raycast_pick(s.g.lo, r.kx); g.lo[1] = raycast_pick(s.g.lo, r.ky); g.lo[2] = raycast_pick(s.g.lo, r.kz);
                g.n[0] = raycast_pick(s.g.n, r.kx); g.n[1] = raycast_pick(s.g.n, r.ky); g.n[2] = raycast_pick(s.g.n, r.kz);
                const double st = slack / fabs(dz), lz = g.lo[2];
                const int c_in = nearest_cell_of(g, 2, r.oz + ta * dz), c_out = nearest_cell_of(g, 2, r.oz + tb * dz);
                const int step = dz > 0.0 ? 1 : -1, w_lo = c_in < c_out ? c_in : c_out, w_hi = c_in < c_out ? c_out : c_in;
                // the strides of the cell id along kx, ky and kz
                const long long s2 = 1, s1 = s.g.n[2], s0 = (long long)s.g.n[1] * s.g.n[2];
                const long long sx = r.kx == 0 ? s0 : (r.kx == 1 ? s1 : s2), sy = r.ky == 0 ? s0 : (r.ky == 1 ? s1 : s2);
                const long long sz = r.kz == 0 ? s0 : (r.kz == 1 ? s1 : s2);
                for (int k = c_in, left = w_hi - w_lo; left >= 0; k += step, --left) {
                    const double tp = ((lz + (double)(step > 0 ? k + 1 : k) * s.g.h) - r.oz) / dz;       // the slab's far plane
                    const double tn = ((lz + (double)(step > 0 ? k : k + 1) * s.g.h) - r.oz) / dz;       // and its near plane
                    const double t_near = k == c_in ? ta : fmax(ta, tn - st);
                    double t_far = k == c_out ? tb : fmin(tb, tp + st);
                    if (FIRST) t_far = fmin(t_far, best.t + st);
                    if (t_near <= t_far) {
                        const double x0 = r.ox + t_near * dx, x1 = r.ox + t_far * dx, y0 = r.oy + t_near * dy, y1 = r.oy + t_far * dy;
                        const int i0 = nearest_cell_of(g, 0, fmin(x0, x1) - slack), i1 = nearest_cell_of(g, 0, fmax(x0, x1) + slack);
                        const int j0 = nearest_cell_of(g, 1, fmin(y0, y1) - slack), j1 = nearest_cell_of(g, 1, fmax(y0, y1) + slack);
                        for (int i = i0; i <= i1; ++i) {
                            for (int j = j0; j <= j1; ++j) {
                                const long long id = s.g.c0 + i * sx + j * sy + k * sz;
                                long long e = cell_start[id];
                                const long long end = cell_start[id + 1];
                                if (e < 0 || end > n_pairs) continue;
                                for (; e < end; ++e) {
                                    const int fl = pair_face[e];
                                    RaycastTerm h;
                                    double flo[3], fhi[3];
                                    if (!raycast_face(verts, faces, s, fl, r, h, flo, fhi, bad)) continue;
                                    if (FIRST) {
                                        if ((cull == 1 && h.sigma > 0) || (cull == 2 && h.sigma < 0)) continue;
                                        if (h.t < best.t || (h.t == best.t && fl < best_face)) {
                                            best = h;
                                            best_face = fl;
                                        }
                                    } else {
                                        // once: in the slab of the hit, clamped to the face's own slabs and to the walk's, and there in
                                        // the first cell of the slab's rectangle that lists the face
                                        int kh = nearest_cell_of(g, 2, r.oz + h.t * dz);
                                        kh = raycast_clamp(kh, nearest_cell_of(g, 2, flo[2]), nearest_cell_of(g, 2, fhi[2]));
                                        kh = raycast_clamp(kh, w_lo, w_hi);
                                        const int fi = nearest_cell_of(g, 0, flo[0]), fj = nearest_cell_of(g, 1, flo[1]);
                                        if (kh == k && (fi > i0 ? fi : i0) == i && (fj > j0 ? fj : j0) == j) {
                                            n_signed += h.sigma;
                                            n_total += 1;
                                        }
                                    }
                                }
                            }
                        }
                    }
                    if (FIRST && best.t < tp - st) break;
                }
            }
        }
    }
    if (FIRST) {
        const bool hit = best_face >= 0;
        out_face[q] = best_face;
        out_t[q] = best.t;
        out_w[q * 3] = hit ? (float)(best.U / best.det) : 0.f;
        out_w[q * 3 + 1] = hit ? (float)(best.V / best.det) : 0.f;
        out_w[q * 3 + 2] = hit ? (float)(best.W / best.det) : 0.f;
        out_side[q] = (signed char)-best.sigma;
    } else {
        out_signed[q] = n_signed;
        out_total[q] = n_total;
    }
}

// the sizes and pointers both entry points check
inline int raycast_args(const float* verts, const int32_t* faces, const int64_t* vert_offset, const int64_t* face_offset, const float* rays_o,
                        const float* rays_d, const int64_t* ray_offset, const float* t_min, const float* t_max, const float* cell,
                        const float* grid_lo, const float* grid_hi, const int64_t* cell_offset, const int64_t* cell_start,
                        const int32_t* pair_face, int64_t n_objects, int64_t n_verts, int64_t n_faces, int64_t n_rays, int64_t n_cells,
                        int64_t n_pairs, const int32_t* bad) {
    int rc = packed_sizes(n_objects, n_verts, n_faces);
    if (rc != SNR_OK) return rc;
    rc = packed_sizes(0, n_rays, 0);
    if (rc != SNR_OK) return rc;
    rc = packed_sizes(0, n_cells, n_pairs);
    if (rc != SNR_OK) return rc;
    if (!bad) return SNR_E_ARG;
    if (n_rays == 0) return SNR_OK;
    if (n_objects == 0 || !vert_offset || !face_offset || !cell || !grid_lo || !grid_hi || !cell_offset || !cell_start) return SNR_E_ARG;
    if ((n_faces && (!faces || !verts)) || (n_pairs && !pair_face)) return SNR_E_ARG;
    if (!rays_o || !rays_d || !ray_offset || !t_min || !t_max) return SNR_E_ARG;
    return SNR_OK;
}

}  // namespace snr

using namespace snr;

extern "C" {

int snr_raycast_first(const float* verts, const int32_t* faces, const int64_t* vert_offset, const int64_t* face_offset, const float* rays_o,
                      const float* rays_d, const int64_t* ray_offset, const float* t_min, const float* t_max, const float* cell,
                      const float* grid_lo, const float* grid_hi, const int64_t* cell_offset, const int64_t* cell_start,
                      const int32_t* pair_face, int64_t n_objects, int64_t n_verts, int64_t n_faces, int64_t n_rays, int64_t n_cells,
                      int64_t n_pairs, int cull, int32_t* face, double* t, float* weights, int8_t* side, int32_t* bad, void* stream) {
    const int rc = raycast_args(verts, faces, vert_offset, face_offset, rays_o, rays_d, ray_offset, t_min, t_max, cell, grid_lo, grid_hi,
                                cell_offset, cell_start, pair_face, n_objects, n_verts, n_faces, n_rays, n_cells, n_pairs, bad);
    if (rc != SNR_OK) return rc;
    if (cull < 0 || cull > 2) return SNR_E_ARG;
    if (n_rays == 0) return SNR_OK;
    if (!face || !t || !weights || !side) return SNR_E_ARG;
    raycast_kernel<true><<<grid_blocks(n_rays), GRID_THREADS, 0, (hipStream_t)stream>>>(
        verts, faces, (const long long*)vert_offset, (const long long*)face_offset, rays_o, rays_d, (const long long*)ray_offset, t_min, t_max,
        cull, cell, grid_lo, grid_hi, (const long long*)cell_offset, (const long long*)cell_start, pair_face, n_objects, n_verts, n_faces,
        n_rays, n_cells, n_pairs, face, t, weights, (signed char*)side, nullptr, nullptr, bad);
    return snr_check_launch_();
}

int snr_raycast_crossings(const float* verts, const int32_t* faces, const int64_t* vert_offset, const int64_t* face_offset,
                          const float* rays_o, const float* rays_d, const int64_t* ray_offset, const float* t_min, const float* t_max,
                          const float* cell, const float* grid_lo, const float* grid_hi, const int64_t* cell_offset,
                          const int64_t* cell_start, const int32_t* pair_face, int64_t n_objects, int64_t n_verts, int64_t n_faces,
                          int64_t n_rays, int64_t n_cells, int64_t n_pairs, int32_t* signed_count, int32_t* total, int32_t* bad,
                          void* stream) {
    const int rc = raycast_args(verts, faces, vert_offset, face_offset, rays_o, rays_d, ray_offset, t_min, t_max, cell, grid_lo, grid_hi,
                                cell_offset, cell_start, pair_face, n_objects, n_verts, n_faces, n_rays, n_cells, n_pairs, bad);
    if (rc != SNR_OK) return rc;
    if (n_rays == 0) return SNR_OK;
    if (!signed_count || !total) return SNR_E_ARG;
    raycast_kernel<false><<<grid_blocks(n_rays), GRID_THREADS, 0, (hipStream_t)stream>>>(
        verts, faces, (const long long*)vert_offset, (const long long*)face_offset, rays_o, rays_d, (const long long*)ray_offset, t_min, t_max,
        0, cell, grid_lo, grid_hi, (const long long*)cell_offset, (const long long*)cell_start, pair_face, n_objects, n_verts, n_faces, n_rays,
        n_cells, n_pairs, nullptr, nullptr, nullptr, nullptr, signed_count, total, bad);
    return snr_check_launch_();
}

}  // extern "C"
