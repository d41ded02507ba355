// Mesh simplification: quadric vertex clustering (Lindstrom 2000) of a packed triangle mesh.
//
// The rules are the header's (include/supnerf_hip.h, "Mesh simplification"); tests/simplify_restatement.py restates them in numpy.  In
// short: every object lays a grid of cubic cells over its vertices, all vertices of a cell become one new vertex, a face survives iff its
// three corners land in three different cells.  The new vertex sits at the mean of its members, or (quadric placement) where the planes
// of every original face that touches the cluster are closest in the least-squares sense, pulled towards the mean by a small ridge term
// and kept inside the cell.
//
// One pass over vertices (keys), one over faces (remap), one over the member and corner lists (sums).  The caller sorts: the vertices by
// (object, cell), the face corners by (cluster, corner index).  Every float64 sum walks its sorted list in slabs of 4096 and fixed trees,
// the segmented sum of snr_packed_mesh.hpp, so the output has the same bits from run to run; there is no floating-point atomic anywhere,
// and no launch reads what another thread of the same launch wrote.
#include "snr_packed_mesh.hpp"
#include "snr_host.hpp"

namespace snr {

constexpr int SIMPLIFY_Q_BITS = 21;                    // bits per axis of the packed key
constexpr int SIMPLIFY_Q_BIAS = 1 << 20;               // |q| < 2^20, so q + bias fits 21 bits

// ---- rule 1: the cell of a vertex.  (x - origin) and the division each round once; false where the cell index is not usable.
__device__ __forceinline__ bool simplify_cell_of(const float* __restrict__ p, const float* __restrict__ org, float cell, int q[3]) {
    bool ok = cell > 0.f && cell <= 3.4028234e38f;
    for (int a = 0; a < 3; ++a) {
        const float d = p[a] - org[a];
        const float qf = floorf(__fdiv_rn(d, cell));
        const bool in = fabsf(qf) < (float)SIMPLIFY_Q_BIAS;               // (false for NaN and infinities too)
        ok = ok && in;
        q[a] = in ? (int)qf : 0;                                          // (-0.f -> 0)
    }
    return ok;
}

__global__ void simplify_keys_kernel(const float* __restrict__ verts, const long long* __restrict__ voff, const float* __restrict__ cell,
                                     const float* __restrict__ origin, long long B, long long nV, long long* __restrict__ key, int* bad) {
    const long long g = grid_thread();
    if (g >= nV) return;
    const long long b = mesh_entry_of(voff, B, g);
    int q[3];
    long long k = 0;
    if (simplify_cell_of(verts + g * 3, origin + b * 3, cell[b], q)) {
        for (int a = 0; a < 3; ++a) k = (k << SIMPLIFY_Q_BITS) | (long long)(q[a] + SIMPLIFY_Q_BIAS);
    } else {
        __hip_atomic_store(bad, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    key[g] = k;
}

// ---- rule 6: the faces under the vertex map
__global__ void simplify_faces_kernel(const int* __restrict__ faces, const int* __restrict__ vert_map, const long long* __restrict__ voff,
                                      const long long* __restrict__ foff, long long B, long long nV, long long nF,
                                      int* __restrict__ new_faces, unsigned char* __restrict__ keep, int* bad) {
    const long long f = grid_thread();
    if (f >= nF) return;
    const MeshFace m = mesh_face(faces, voff, foff, B, nV, f);
    int n[3] = {-1, -1, -1};
    bool k = false;
    if (m.ok) {
        for (int a = 0; a < 3; ++a) n[a] = vert_map[m.v0 + m.idx[a]];
        k = n[0] != n[1] && n[1] != n[2] && n[0] != n[2];
    } else {
        __hip_atomic_store(bad, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (int a = 0; a < 3; ++a) new_faces[f * 3 + a] = n[a];
    keep[f] = k;
}

// kept faces to the front, in their original order: face f goes to slot keep_scan[f] - 1 (keep_scan: the inclusive scan of keep)
__global__ void simplify_compact_kernel(const int* __restrict__ new_faces, const unsigned char* __restrict__ keep,
                                        const long long* __restrict__ keep_scan, long long nF, long long n_kept, int* __restrict__ out_faces,
                                        long long* __restrict__ face_index) {
    const long long f = grid_thread();
    if (f >= nF || !keep[f]) return;
    const long long s = keep_scan[f] - 1;
    if (s < 0 || s >= n_kept) return;
    for (int k = 0; k < 3; ++k) out_faces[s * 3 + k] = new_faces[f * 3 + k];
    face_index[s] = f;
}

// ---- rule 5: every sum below is the fixed-order segmented sum of snr_packed_mesh.hpp (segment_slab, block_tree, wave_sum)

// the members' coordinates, widened: partial (n_slabs, 3)
__global__ void __launch_bounds__(GRID_THREADS) simplify_vert_slab_kernel(const float* __restrict__ verts,
                                                                          const long long* __restrict__ vert_order,
                                                                          const long long* __restrict__ seg_start,
                                                                          const long long* __restrict__ slab_off, long long nC, long long nV,
                                                                          double* __restrict__ partial) {
    __shared__ double s_sum[3 * GRID_THREADS];
    const SegmentSlab sl = segment_slab(seg_start, slab_off, nC, nV);
    if (sl.c < 0) return;                                                    // (uniform over the block)
    double acc[3] = {0.0, 0.0, 0.0};
    for (long long i = sl.begin + threadIdx.x; i < sl.end; i += GRID_THREADS) {
        const long long g = vert_order[i];
        if (g < 0 || g >= nV) continue;
        for (int a = 0; a < 3; ++a) acc[a] += (double)verts[g * 3 + a];
    }
    block_tree<3>(acc, s_sum, partial + (long long)blockIdx.x * 3);
}

// the object and the cell of cluster k, from its first member in the sorted order (rule 1 again: the same operations, the same bits)
struct SimplifyCell {
    bool ok;
    double cell, org[3], q[3];        // the cell edge, the origin and the cell index, widened
    // origin + (q + t) cell: t = 0 and 1 are the faces of the cell, t = 1/2 its centre c0
    __device__ __forceinline__ double at(int a, double t) const { return org[a] + (q[a] + t) * cell; }
};
__device__ __forceinline__ SimplifyCell simplify_cluster_cell(const float* __restrict__ verts, const long long* __restrict__ vert_order,
                                                              const long long* __restrict__ vseg_start, const long long* __restrict__ voff,
                                                              const float* __restrict__ cell, const float* __restrict__ origin, long long B,
                                                              long long nV, long long k) {
    SimplifyCell r;
    r.ok = false;
    r.cell = 0.0;
    for (int a = 0; a < 3; ++a) r.org[a] = r.q[a] = 0.0;
    const long long i0 = vseg_start[k];
    if (i0 < 0 || i0 >= nV) return r;
    const long long g = vert_order[i0];
    if (g < 0 || g >= nV) return r;
    const long long b = mesh_entry_of(voff, B, g);
    int q[3];
    if (!simplify_cell_of(verts + g * 3, origin + b * 3, cell[b], q)) return r;
    r.ok = true;
    r.cell = (double)cell[b];
    for (int a = 0; a < 3; ++a) { r.org[a] = (double)origin[b * 3 + a]; r.q[a] = (double)q[a]; }
    return r;
}

// rule 4: the nine quadric sums over the cluster's (face, corner) pairs, n and d formed on the fly: partial (n_slabs, 9) =
// A00 A01 A02 A11 A12 A22 v0 v1 v2
__global__ void __launch_bounds__(GRID_THREADS) simplify_corner_slab_kernel(
    const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
    const float* __restrict__ cell, const float* __restrict__ origin, long long B, long long nV, long long nF,
    const long long* __restrict__ vert_order, const long long* __restrict__ vseg_start, const long long* __restrict__ corner_order,
    const long long* __restrict__ cseg_start, const long long* __restrict__ cslab_off, long long nC, double* __restrict__ partial) {
    __shared__ double s_sum[9 * GRID_THREADS];
    const SegmentSlab sl = segment_slab(cseg_start, cslab_off, nC, nF * 3);
    if (sl.c < 0) return;
    const SimplifyCell cc = simplify_cluster_cell(verts, vert_order, vseg_start, voff, cell, origin, B, nV, sl.c);
    double c0[3];
    for (int a = 0; a < 3; ++a) c0[a] = cc.at(a, 0.5);
    double acc[9];
    for (int j = 0; j < 9; ++j) acc[j] = 0.0;
    for (long long i = sl.begin + threadIdx.x; i < sl.end && cc.ok; i += GRID_THREADS) {
        const long long corner = corner_order[i];
        if (corner < 0 || corner >= nF * 3) continue;
        const MeshFace m = mesh_face(faces, voff, foff, B, nV, corner / 3);
        if (!m.ok) continue;
        double pa[3], e1[3], e2[3];
        for (int a = 0; a < 3; ++a) {
            pa[a] = (double)verts[(m.v0 + m.idx[0]) * 3 + a] - c0[a];
            e1[a] = ((double)verts[(m.v0 + m.idx[1]) * 3 + a] - c0[a]) - pa[a];
            e2[a] = ((double)verts[(m.v0 + m.idx[2]) * 3 + a] - c0[a]) - pa[a];
        }
        double n[3];
        n[0] = e1[1] * e2[2] - e1[2] * e2[1];
        n[1] = e1[2] * e2[0] - e1[0] * e2[2];
        n[2] = e1[0] * e2[1] - e1[1] * e2[0];
        const double d = -((n[0] * pa[0] + n[1] * pa[1]) + n[2] * pa[2]);
        acc[0] += n[0] * n[0]; acc[1] += n[0] * n[1]; acc[2] += n[0] * n[2];
        acc[3] += n[1] * n[1]; acc[4] += n[1] * n[2]; acc[5] += n[2] * n[2];
        acc[6] += d * n[0]; acc[7] += d * n[1]; acc[8] += d * n[2];
    }
    block_tree<9>(acc, s_sum, partial + (long long)blockIdx.x * 9);
}

// (A + lambda I) y = r for a symmetric positive definite A + lambda I, by Cholesky; a = A00 A01 A02 A11 A12 A22
__device__ __forceinline__ void simplify_solve(const double* a, double lambda, const double* r, double* y) {
    const double l00 = sqrt(a[0] + lambda);
    const double l10 = a[1] / l00, l20 = a[2] / l00;
    const double l11 = sqrt((a[3] + lambda) - l10 * l10);
    const double l21 = (a[4] - l20 * l10) / l11;
    const double l22 = sqrt(((a[5] + lambda) - l20 * l20) - l21 * l21);
    const double z0 = r[0] / l00;
    const double z1 = (r[1] - l10 * z0) / l11;
    const double z2 = ((r[2] - l20 * z0) - l21 * z1) / l22;
    y[2] = z2 / l22;
    y[1] = (z1 - l21 * y[2]) / l11;
    y[0] = ((z0 - l10 * y[1]) - l20 * y[2]) / l00;
}

// a wave per cluster: the slab sums in their order, then rule 3 or rule 4 by lane 0
__global__ void simplify_cluster_kernel(const float* __restrict__ verts, const long long* __restrict__ voff, const float* __restrict__ cell,
                                        const float* __restrict__ origin, long long B, long long nV,
                                        const long long* __restrict__ vert_order, const long long* __restrict__ vseg_start,
                                        const long long* __restrict__ vslab_off, const long long* __restrict__ cslab_off, long long nC,
                                        const double* __restrict__ vpartial, long long n_vslabs, const double* __restrict__ cpartial,
                                        long long n_cslabs, int quadric, float* __restrict__ out) {
    const long long gid = grid_thread();
    const long long k = gid >> 6;
    const int lane = (int)(gid & 63);
    if (k >= nC) return;                                                     // (whole waves: 256 threads per block, 64 per cluster)
    double sv[3], sq[9];
    wave_sum<3>(vpartial, 3, vslab_off[k], vslab_off[k + 1], n_vslabs, lane, sv);
    for (int j = 0; j < 9; ++j) sq[j] = 0.0;
    if (quadric) wave_sum<9>(cpartial, 9, cslab_off[k], cslab_off[k + 1], n_cslabs, lane, sq);
    if (lane != 0) return;
    const long long count = vseg_start[k + 1] - vseg_start[k];
    double m[3], x[3];
    for (int a = 0; a < 3; ++a) x[a] = m[a] = sv[a] / (double)(count > 0 ? count : 1);
    if (quadric) {
        const SimplifyCell cc = simplify_cluster_cell(verts, vert_order, vseg_start, voff, cell, origin, B, nV, k);
        const double tr = (sq[0] + sq[3]) + sq[5];
        const double tiny = 1e-12 * cc.cell * cc.cell;
        if (cc.ok && tr > tiny * tiny) {
            const double lambda = SNR_SIMPLIFY_EPS * tr;
            double r[3], y[3];
            for (int a = 0; a < 3; ++a) r[a] = lambda * (m[a] - cc.at(a, 0.5)) - sq[6 + a];
            simplify_solve(sq, lambda, r, y);
            for (int a = 0; a < 3; ++a) {
                const double lo = cc.at(a, 0.0), hi = cc.at(a, 1.0);
                double v = cc.at(a, 0.5) + y[a];
                v = v < lo ? lo : v;                                         // (a NaN goes to hi: the output stays finite)
                x[a] = v <= hi ? v : hi;
            }
        }
    }
    for (int a = 0; a < 3; ++a) out[k * 3 + a] = (float)x[a];
}

// ---- rule 7: attribute means over the same vertex segments: partial (n_slabs, C), blockIdx.y = channel
__global__ void __launch_bounds__(GRID_THREADS) simplify_attr_slab_kernel(const float* __restrict__ attr, int C,
                                                                          const long long* __restrict__ vert_order,
                                                                          const long long* __restrict__ seg_start,
                                                                          const long long* __restrict__ slab_off, long long nC, long long nV,
                                                                          double* __restrict__ partial) {
    __shared__ double s_sum[GRID_THREADS];
    const SegmentSlab sl = segment_slab(seg_start, slab_off, nC, nV);
    if (sl.c < 0) return;
    const int ch = blockIdx.y;
    double acc[1] = {0.0};
    for (long long i = sl.begin + threadIdx.x; i < sl.end; i += GRID_THREADS) {
        const long long g = vert_order[i];
        if (g < 0 || g >= nV) continue;
        acc[0] += (double)attr[g * C + ch];
    }
    block_tree<1>(acc, s_sum, partial + (long long)blockIdx.x * C + ch);
}

// a wave per (cluster, channel)
__global__ void simplify_attr_cluster_kernel(const double* __restrict__ partial, int C, const long long* __restrict__ seg_start,
                                             const long long* __restrict__ slab_off, long long nC, long long n_slabs,
                                             float* __restrict__ out) {
    const long long gid = grid_thread();
    const long long w = gid >> 6;
    const int lane = (int)(gid & 63);
    if (w >= nC * C) return;
    const long long k = w / C;
    const int ch = (int)(w - k * C);
    double a[1];
    wave_sum<1>(partial + ch, C, slab_off[k], slab_off[k + 1], n_slabs, lane, a);
    const long long count = seg_start[k + 1] - seg_start[k];
    if (lane == 0) out[k * C + ch] = (float)(a[0] / (double)(count > 0 ? count : 1));
}

}  // namespace snr

using namespace snr;

extern "C" {

int snr_simplify_keys(const float* verts, const int64_t* vert_offset, const float* cell, const float* origin, int64_t n_objects,
                      int64_t n_verts, int64_t* key, int32_t* bad, void* stream) {
    const int rc = packed_sizes(n_objects, n_verts, 0);
    if (rc != SNR_OK) return rc;
    if (!bad) return SNR_E_ARG;
    if (n_verts == 0) return SNR_OK;
    if (n_objects == 0 || !verts || !vert_offset || !cell || !origin || !key) return SNR_E_ARG;
    simplify_keys_kernel<<<grid_blocks(n_verts), GRID_THREADS, 0, (hipStream_t)stream>>>(verts, (const long long*)vert_offset, cell, origin,
                                                                                        n_objects, n_verts, (long long*)key, bad);
    return snr_check_launch_();
}

int snr_simplify_faces(const int32_t* faces, const int32_t* vert_map, const int64_t* vert_offset, const int64_t* face_offset,
                       int64_t n_objects, int64_t n_verts, int64_t n_faces, int32_t* new_faces, uint8_t* keep, int32_t* bad, void* stream) {
    const int rc = packed_sizes(n_objects, n_verts, n_faces);
    if (rc != SNR_OK) return rc;
    if (!bad) return SNR_E_ARG;
    if (n_faces == 0) return SNR_OK;
    if (n_objects == 0 || !faces || !vert_offset || !face_offset || !new_faces || !keep || (n_verts && !vert_map)) return SNR_E_ARG;
    simplify_faces_kernel<<<grid_blocks(n_faces), GRID_THREADS, 0, (hipStream_t)stream>>>(
        faces, vert_map, (const long long*)vert_offset, (const long long*)face_offset, n_objects, n_verts, n_faces, new_faces, keep, bad);
    return snr_check_launch_();
}

int snr_simplify_compact(const int32_t* new_faces, const uint8_t* keep, const int64_t* keep_scan, int64_t n_faces, int64_t n_kept,
                         int32_t* out_faces, int64_t* face_index, void* stream) {
    const int rc = packed_sizes(0, n_faces, n_kept);
    if (rc != SNR_OK) return rc;
    if (n_kept > n_faces) return SNR_E_ARG;
    if (n_faces == 0 || n_kept == 0) return SNR_OK;
    if (!new_faces || !keep || !keep_scan || !out_faces || !face_index) return SNR_E_ARG;
    simplify_compact_kernel<<<grid_blocks(n_faces), GRID_THREADS, 0, (hipStream_t)stream>>>(new_faces, keep, (const long long*)keep_scan,
                                                                                           n_faces, n_kept, out_faces, (long long*)face_index);
    return snr_check_launch_();
}

int snr_simplify_positions(const float* verts, const int32_t* faces, const int64_t* vert_offset, const int64_t* face_offset,
                           const float* cell, const float* origin, int64_t n_objects, int64_t n_verts, int64_t n_faces,
                           const int64_t* vert_order, const int64_t* vert_seg_start, const int64_t* vert_slab_offset,
                           const int64_t* corner_order, const int64_t* corner_seg_start, const int64_t* corner_slab_offset,
                           int64_t n_clusters, int quadric, double* vert_partial, int64_t n_vert_slabs, double* corner_partial,
                           int64_t n_corner_slabs, float* out_verts, void* stream) {
    int rc = packed_sizes(n_objects, n_verts, n_faces);
    if (rc != SNR_OK) return rc;
    rc = packed_sizes(0, n_clusters, 0);
    if (rc != SNR_OK) return rc;
    if (n_vert_slabs < 0 || n_corner_slabs < 0 || (quadric != 0 && quadric != 1) || n_clusters > n_verts) return SNR_E_ARG;
    if (n_clusters == 0) return SNR_OK;
    const bool corners = quadric && n_faces > 0;
    if (n_vert_slabs < snr_segment_slab_bound(n_clusters, n_verts)) return SNR_E_WORKSPACE;
    if (corners && n_corner_slabs < snr_segment_slab_bound(n_clusters, n_faces * 3)) return SNR_E_WORKSPACE;
    if (n_vert_slabs > 0x7fffffffll || n_corner_slabs > 0x7fffffffll || n_clusters > 0x7fffffffll) return SNR_E_UNSUPPORTED;
    if (n_objects == 0 || !verts || !vert_offset || !cell || !origin || !vert_order || !vert_seg_start || !vert_slab_offset ||
        !vert_partial || !out_verts)
        return SNR_E_ARG;
    if (corners && (!faces || !face_offset || !corner_order || !corner_seg_start || !corner_slab_offset || !corner_partial)) return SNR_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const long long* voff = (const long long*)vert_offset;
    const long long* vorder = (const long long*)vert_order;
    const long long* vseg = (const long long*)vert_seg_start;
    const long long* vslab = (const long long*)vert_slab_offset;
    simplify_vert_slab_kernel<<<(unsigned)n_vert_slabs, GRID_THREADS, 0, st>>>(verts, vorder, vseg, vslab, n_clusters, n_verts, vert_partial);
    if (corners)
        simplify_corner_slab_kernel<<<(unsigned)n_corner_slabs, GRID_THREADS, 0, st>>>(
            verts, faces, voff, (const long long*)face_offset, cell, origin, n_objects, n_verts, n_faces, vorder, vseg,
            (const long long*)corner_order, (const long long*)corner_seg_start, (const long long*)corner_slab_offset, n_clusters,
            corner_partial);
    simplify_cluster_kernel<<<grid_blocks(n_clusters * 64), GRID_THREADS, 0, st>>>(
        verts, voff, cell, origin, n_objects, n_verts, vorder, vseg, vslab, (const long long*)corner_slab_offset, n_clusters, vert_partial,
        n_vert_slabs, corner_partial, n_corner_slabs, corners ? 1 : 0, out_verts);
    return snr_check_launch_();
}

int snr_simplify_attributes(const float* attributes, int n_channels, int64_t n_verts, const int64_t* vert_order,
                            const int64_t* vert_seg_start, const int64_t* vert_slab_offset, int64_t n_clusters, double* partial,
                            int64_t n_slabs, float* out, void* stream) {
    const int rc = packed_sizes(0, n_verts, n_clusters);
    if (rc != SNR_OK) return rc;
    if (n_channels < 1 || n_channels > PACKED_MAX_CHANNELS || n_slabs < 0 || n_clusters > n_verts) return SNR_E_ARG;
    if (n_clusters == 0) return SNR_OK;
    if (n_slabs < snr_segment_slab_bound(n_clusters, n_verts)) return SNR_E_WORKSPACE;
    if (n_slabs > 0x7fffffffll || n_clusters * n_channels > (0x7fffffffll >> 2)) return SNR_E_UNSUPPORTED;
    if (!attributes || !vert_order || !vert_seg_start || !vert_slab_offset || !partial || !out) return SNR_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const long long* vseg = (const long long*)vert_seg_start;
    const long long* vslab = (const long long*)vert_slab_offset;
    simplify_attr_slab_kernel<<<dim3((unsigned)n_slabs, (unsigned)n_channels), GRID_THREADS, 0, st>>>(
        attributes, n_channels, (const long long*)vert_order, vseg, vslab, n_clusters, n_verts, partial);
    simplify_attr_cluster_kernel<<<grid_blocks(n_clusters * n_channels * 64), GRID_THREADS, 0, st>>>(partial, n_channels, vseg, vslab,
                                                                                                    n_clusters, n_slabs, out);
    return snr_check_launch_();
}

}  // extern "C"
