// Mesh components: which vertices and faces of a packed triangle mesh hang together, and what each piece measures.
//
// The rules are the header's (include/supnerf_hip.h, "Mesh components"); tests/mesh_restatement.py restates them in numpy.  In short: two
// vertices are connected iff a chain of faces links them through shared vertex indices; component c of an object is the one whose smallest
// vertex index is the c-th smallest; per component the vertex and face counts, the bounding box, the area and the signed volume about its
// vertex of smallest index, both summed in float64 in a fixed order.
//
// The union is a lock-free union-find over the face list (ECL-CC style hooking: the larger root always goes under the smaller, so the final
// root of a component is its smallest vertex index).  MI355X has eight XCDs whose L2s are not coherent with each other, so inside the hook
// launch EVERY read of the parent array is an agent-scope atomic load and every update an agent-scope compare-and-swap or atomic min; plain
// loads of it happen only in later launches (mesh_flatten_kernel), plain stores only in the launch before (mesh_identity_kernel).  A stale
// parent is still an ancestor, and a compare-and-swap that fails retries on the value it returned: no thread ever waits for another one.
// Nothing here adds floating-point numbers atomically: counts and boxes use integer atomics (exact, whatever the order), the float64 sums
// walk the faces sorted by component in the fixed order of snr_packed_mesh.hpp, so every output has the same bits from run to run.
#include "snr_packed_mesh.hpp"
#include "snr_host.hpp"

namespace snr {

#define SNR_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__global__ void mesh_identity_kernel(const long long* __restrict__ voff, long long B, long long nV, int* __restrict__ parent) {
    const long long g = grid_thread();
    if (g >= nV) return;
    parent[g] = (int)(g - voff[mesh_entry_of(voff, B, g)]);
}

// ---- the hook launch: every access to `par` below is an agent-scope atomic
__device__ __forceinline__ int mesh_par_load(const int* par, int x) { return __hip_atomic_load(par + x, SNR_RLX_AGENT); }

// the root above x; on the way every visited vertex is pointed at its grandparent (an atomic min: parents only ever decrease)
__device__ __forceinline__ int mesh_find(int* par, int x) {
    int p = mesh_par_load(par, x);
    while (p != x) {
        const int gp = mesh_par_load(par, p);
        if (gp != p) __hip_atomic_fetch_min(par + x, gp, SNR_RLX_AGENT);
        x = p;
        p = gp;
    }
    return x;
}

__device__ __forceinline__ void mesh_unite(int* par, int u, int v) {
    for (;;) {
        u = mesh_find(par, u);
        v = mesh_find(par, v);
        if (u == v) return;
        const int hi = u > v ? u : v, lo = u > v ? v : u;
        int expected = hi;
        if (__hip_atomic_compare_exchange_strong(par + hi, &expected, lo, __ATOMIC_RELAXED, SNR_RLX_AGENT)) return;      // hi was a root: now under lo
        u = expected;                 // hi had been hooked meanwhile: `expected` is its parent, an ancestor -- go on from there
        v = lo;
    }
}

__global__ void mesh_hook_kernel(const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
                                 long long B, long long nV, long long nF, int* parent, int* bad) {
    const long long f = grid_thread();
    if (f >= nF) return;
    const MeshFace m = mesh_face(faces, voff, foff, B, nV, f);
    if (!m.ok) { __hip_atomic_store(bad, 1, SNR_RLX_AGENT); return; }
    int* par = parent + m.v0;
    mesh_unite(par, m.idx[0], m.idx[1]);
    mesh_unite(par, m.idx[0], m.idx[2]);
}

// ---- later launches: the parent array is final and read with plain loads
__global__ void mesh_flatten_kernel(const int* __restrict__ parent, const long long* __restrict__ voff, long long B, long long nV,
                                    int* __restrict__ root, unsigned char* __restrict__ is_root) {
    const long long g = grid_thread();
    if (g >= nV) return;
    const long long v0 = voff[mesh_entry_of(voff, B, g)];
    const int* par = parent + v0;
    const int v = (int)(g - v0);
    int r = v, p = par[r];
    while (p < r) {                   // (a parent is never larger than its child; p == r is the root)
        r = p;
        p = par[r];
    }
    root[g] = r;
    is_root[g] = r == v;
}

__global__ void mesh_vert_label_kernel(const int* __restrict__ root, const int* __restrict__ root_scan, const long long* __restrict__ voff,
                                       long long B, long long nV, int* __restrict__ vert_label) {
    const long long g = grid_thread();
    if (g >= nV) return;
    const long long v0 = voff[mesh_entry_of(voff, B, g)];
    vert_label[g] = root_scan[v0 + root[g]] - 1;
}

__global__ void mesh_face_label_kernel(const int* __restrict__ faces, const int* __restrict__ vert_label, const long long* __restrict__ voff,
                                       const long long* __restrict__ foff, long long B, long long nV, long long nF,
                                       int* __restrict__ face_label) {
    const long long f = grid_thread();
    if (f >= nF) return;
    const MeshObject o = mesh_object(voff, mesh_entry_of(foff, B, f), nV);
    const int i0 = faces[f * 3];
    face_label[f] = mesh_index_ok(i0, o.V) ? vert_label[o.v0 + i0] : -1;
}

// ---- counts and boxes: integer atomics on order-preserving keys of the coordinates
__device__ __forceinline__ unsigned mesh_float_key(float x) {
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float mesh_key_float(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

struct MeshBox {
    unsigned lo[3], hi[3], n;
};
__device__ __forceinline__ void mesh_box_merge(MeshBox& a, const MeshBox& b) {
    for (int k = 0; k < 3; ++k) {
        a.lo[k] = a.lo[k] < b.lo[k] ? a.lo[k] : b.lo[k];
        a.hi[k] = a.hi[k] > b.hi[k] ? a.hi[k] : b.hi[k];
    }
    a.n += b.n;
}
__device__ __forceinline__ void mesh_box_commit(const MeshBox& x, long long c, unsigned long long* cnt, unsigned* lo, unsigned* hi) {
    atomicAdd(cnt + c, (unsigned long long)x.n);
    for (int k = 0; k < 3; ++k) {
        atomicMin(lo + c * 3 + k, x.lo[k]);
        atomicMax(hi + c * 3 + k, x.hi[k]);
    }
}

__global__ void mesh_box_init_kernel(long long nC, unsigned long long* __restrict__ cnt, unsigned* __restrict__ lo, unsigned* __restrict__ hi) {
    const long long c = grid_thread();
    if (c >= nC) return;
    cnt[c] = 0;
    for (int k = 0; k < 3; ++k) {
        lo[c * 3 + k] = 0xffffffffu;
        hi[c * 3 + k] = 0u;
    }
}

// One thread per vertex.  Neighbouring vertices mostly share a component (one giant piece is the common case), so the lanes of a wave
// that hold the same component are merged by shuffles first and one lane commits for them; the group of each wave's first lane goes
// through LDS, where thread 0 merges the workgroup's four before it commits.  Integer min / max / add: the result is exact in any order.
__global__ void __launch_bounds__(GRID_THREADS) mesh_box_kernel(const float* __restrict__ verts, const int* __restrict__ vert_label,
                                                                const long long* __restrict__ voff, const long long* __restrict__ coff,
                                                                long long B, long long nV, long long nC, unsigned long long* cnt,
                                                                unsigned* lo, unsigned* hi) {
    __shared__ long long s_c[GRID_THREADS / 64];
    __shared__ MeshBox s_box[GRID_THREADS / 64];
    const long long g = grid_thread();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    long long c = -1;
    MeshBox mine;
    for (int k = 0; k < 3; ++k) { mine.lo[k] = 0xffffffffu; mine.hi[k] = 0u; }
    mine.n = 0;
    if (g < nV) {
        const long long b = mesh_entry_of(voff, B, g);
        c = coff[b] + vert_label[g];
        if (c < coff[b] || c >= coff[b + 1] || c >= nC) c = -1;           // (labels that are not this object's: not counted)
    }
    if (c >= 0) {
        for (int k = 0; k < 3; ++k) mine.lo[k] = mine.hi[k] = mesh_float_key(verts[g * 3 + k]);
        mine.n = 1;
    }
    if (lane == 0) s_c[w] = -1;
    bool first = true;
    unsigned long long left = __ballot(c >= 0);
    while (left) {                                                          // (wave-uniform: every lane takes part in the shuffles)
        const int leader = __ffsll((long long)left) - 1;
        const long long cl = __shfl(c, leader);
        const bool in = c == cl;
        MeshBox x;
        for (int k = 0; k < 3; ++k) { x.lo[k] = in ? mine.lo[k] : 0xffffffffu; x.hi[k] = in ? mine.hi[k] : 0u; }
        x.n = in ? mine.n : 0u;
        for (int s = 32; s; s >>= 1) {
            MeshBox y;
            for (int k = 0; k < 3; ++k) { y.lo[k] = __shfl_xor(x.lo[k], s); y.hi[k] = __shfl_xor(x.hi[k], s); }
            y.n = __shfl_xor(x.n, s);
            mesh_box_merge(x, y);
        }
        if (lane == leader) {
            if (first) { s_c[w] = cl; s_box[w] = x; }
            else mesh_box_commit(x, cl, cnt, lo, hi);
        }
        first = false;
        left &= ~__ballot(in);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int i = 0; i < GRID_THREADS / 64; ++i) {
        if (s_c[i] < 0) continue;
        MeshBox x = s_box[i];
        for (int j = i + 1; j < GRID_THREADS / 64; ++j)
            if (s_c[j] == s_c[i]) { mesh_box_merge(x, s_box[j]); s_c[j] = -1; }
        mesh_box_commit(x, s_c[i], cnt, lo, hi);
    }
}

__global__ void mesh_box_decode_kernel(long long n, unsigned* __restrict__ lo, unsigned* __restrict__ hi) {
    const long long i = grid_thread();
    if (i >= n) return;
    lo[i] = __float_as_uint(mesh_key_float(lo[i]));
    hi[i] = __float_as_uint(mesh_key_float(hi[i]));
}

// ---- area and volume terms, one thread per face, slot i = face order[i] (order: the faces sorted by component; null = as stored)
__global__ void mesh_face_terms_kernel(const float* __restrict__ verts, const int* __restrict__ faces, const int* __restrict__ root,
                                       const long long* __restrict__ order, const long long* __restrict__ voff,
                                       const long long* __restrict__ foff, long long B, long long nV, long long nF,
                                       double* __restrict__ area_t, double* __restrict__ vol_t) {
    const long long i = grid_thread();
    if (i >= nF) return;
    const long long f = order ? order[i] : i;
    double area = 0.0, vol = 0.0;
    if (f >= 0 && f < nF) {
        const MeshFace m = mesh_face(faces, voff, foff, B, nV, f);
        if (m.ok) {
            const float* pa = verts + (m.v0 + m.idx[0]) * 3;
            const float* pb = verts + (m.v0 + m.idx[1]) * 3;
            const float* pc = verts + (m.v0 + m.idx[2]) * 3;
            const float* p0 = verts + (m.v0 + root[m.v0 + m.idx[0]]) * 3;    // the component's vertex of smallest index is its root
            double a[3], b[3], c[3], p[3];
            for (int k = 0; k < 3; ++k) { a[k] = (double)pa[k]; b[k] = (double)pb[k]; c[k] = (double)pc[k]; p[k] = (double)p0[k]; }
            double e1[3], e2[3];
            for (int k = 0; k < 3; ++k) { e1[k] = b[k] - a[k]; e2[k] = c[k] - a[k]; }
            const double nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
            area = sqrt(nx * nx + ny * ny + nz * nz) / 2.0;
            for (int k = 0; k < 3; ++k) { a[k] -= p[k]; b[k] -= p[k]; c[k] -= p[k]; }
            const double cx = b[1] * c[2] - b[2] * c[1], cy = b[2] * c[0] - b[0] * c[2], cz = b[0] * c[1] - b[1] * c[0];
            vol = (a[0] * cx + a[1] * cy + a[2] * cz) / 6.0;
        }
    }
    area_t[i] = area;
    vol_t[i] = vol;
}

// ---- the two float64 sums per component: the fixed-order segmented sum of snr_packed_mesh.hpp with N = 2 (area, volume)
__global__ void __launch_bounds__(GRID_THREADS) mesh_slab_sum_kernel(const double* __restrict__ area_t, const double* __restrict__ vol_t,
                                                                     const long long* __restrict__ seg_start,
                                                                     const long long* __restrict__ slab_off, long long nC, long long nF,
                                                                     double* __restrict__ partial) {
    __shared__ double s_sum[2 * GRID_THREADS];
    const SegmentSlab sl = segment_slab(seg_start, slab_off, nC, nF);
    if (sl.c < 0) return;                                                   // (uniform over the block)
    double acc[2] = {0.0, 0.0};
    for (long long i = sl.begin + threadIdx.x; i < sl.end; i += GRID_THREADS) { acc[0] += area_t[i]; acc[1] += vol_t[i]; }
    block_tree<2>(acc, s_sum, partial + (long long)blockIdx.x * 2);
}

// a wave per component
__global__ void mesh_comp_sum_kernel(const double* __restrict__ partial, const long long* __restrict__ slab_off, long long nC,
                                     long long n_slabs, double* __restrict__ area, double* __restrict__ volume) {
    const long long gid = grid_thread();
    const long long c = gid >> 6;
    const int lane = (int)(gid & 63);
    if (c >= nC) return;                                                    // (whole waves: 256 threads per block, 64 per component)
    double acc[2];
    wave_sum<2>(partial, 2, slab_off[c], slab_off[c + 1], n_slabs, lane, acc);
    if (lane == 0) { area[c] = acc[0]; volume[c] = acc[1]; }
}

}  // namespace snr

using namespace snr;

extern "C" {

int snr_mesh_hook(const int32_t* faces, const int64_t* vert_offset, const int64_t* face_offset, int64_t n_objects, int64_t n_verts,
                  int64_t n_faces, int32_t* parent, int32_t* bad, void* stream) {
    const int rc = packed_sizes(n_objects, n_verts, n_faces);
    if (rc != SNR_OK) return rc;
    if (!bad) return SNR_E_ARG;
    if (n_verts == 0 && n_faces == 0) return SNR_OK;
    if (n_objects == 0 || !vert_offset || !face_offset || (n_verts && !parent) || (n_faces && !faces)) return SNR_E_ARG;
    const long long* voff = (const long long*)vert_offset;
    const long long* foff = (const long long*)face_offset;
    if (n_verts) mesh_identity_kernel<<<grid_blocks(n_verts), GRID_THREADS, 0, (hipStream_t)stream>>>(voff, n_objects, n_verts, parent);
    if (n_faces)
        mesh_hook_kernel<<<grid_blocks(n_faces), GRID_THREADS, 0, (hipStream_t)stream>>>(faces, voff, foff, n_objects, n_verts, n_faces, parent,
                                                                                         bad);
    return snr_check_launch_();
}

int snr_mesh_flatten(const int32_t* parent, const int64_t* vert_offset, int64_t n_objects, int64_t n_verts, int32_t* root, uint8_t* is_root,
                     void* stream) {
    const int rc = packed_sizes(n_objects, n_verts, 0);
    if (rc != SNR_OK) return rc;
    if (n_verts == 0) return SNR_OK;
    if (n_objects == 0 || !parent || !vert_offset || !root || !is_root) return SNR_E_ARG;
    mesh_flatten_kernel<<<grid_blocks(n_verts), GRID_THREADS, 0, (hipStream_t)stream>>>(parent, (const long long*)vert_offset, n_objects,
                                                                                        n_verts, root, is_root);
    return snr_check_launch_();
}

int snr_mesh_label(const int32_t* root, const int32_t* root_scan, const int32_t* faces, const int64_t* vert_offset,
                   const int64_t* face_offset, int64_t n_objects, int64_t n_verts, int64_t n_faces, int32_t* vert_label, int32_t* face_label,
                   void* stream) {
    const int rc = packed_sizes(n_objects, n_verts, n_faces);
    if (rc != SNR_OK) return rc;
    if (n_verts == 0 && n_faces == 0) return SNR_OK;
    if (n_objects == 0 || !vert_offset || !face_offset || (n_verts && (!root || !root_scan || !vert_label)) ||
        (n_faces && (!faces || !face_label || !vert_label)))
        return SNR_E_ARG;
    const long long* voff = (const long long*)vert_offset;
    if (n_verts)
        mesh_vert_label_kernel<<<grid_blocks(n_verts), GRID_THREADS, 0, (hipStream_t)stream>>>(root, root_scan, voff, n_objects, n_verts,
                                                                                               vert_label);
    if (n_faces)
        mesh_face_label_kernel<<<grid_blocks(n_faces), GRID_THREADS, 0, (hipStream_t)stream>>>(faces, vert_label, voff,
                                                                                               (const long long*)face_offset, n_objects,
                                                                                               n_verts, n_faces, face_label);
    return snr_check_launch_();
}

int snr_mesh_boxes(const float* verts, const int32_t* vert_label, const int64_t* vert_offset, const int64_t* comp_offset, int64_t n_objects,
                   int64_t n_verts, int64_t n_comps, int64_t* comp_verts, float* bbox_lo, float* bbox_hi, void* stream) {
    const int rc = packed_sizes(n_objects, n_verts, n_comps);
    if (rc != SNR_OK) return rc;
    if (n_comps == 0) return SNR_OK;
    if (n_objects == 0 || !vert_offset || !comp_offset || !comp_verts || !bbox_lo || !bbox_hi || (n_verts && (!verts || !vert_label)))
        return SNR_E_ARG;
    unsigned long long* cnt = (unsigned long long*)comp_verts;
    unsigned* lo = (unsigned*)bbox_lo;
    unsigned* hi = (unsigned*)bbox_hi;
    hipStream_t st = (hipStream_t)stream;
    mesh_box_init_kernel<<<grid_blocks(n_comps), GRID_THREADS, 0, st>>>(n_comps, cnt, lo, hi);
    if (n_verts)
        mesh_box_kernel<<<grid_blocks(n_verts), GRID_THREADS, 0, st>>>(verts, vert_label, (const long long*)vert_offset,
                                                                       (const long long*)comp_offset, n_objects, n_verts, n_comps, cnt, lo, hi);
    mesh_box_decode_kernel<<<grid_blocks(n_comps * 3), GRID_THREADS, 0, st>>>(n_comps * 3, lo, hi);
    return snr_check_launch_();
}

int snr_mesh_face_terms(const float* verts, const int32_t* faces, const int32_t* root, const int64_t* order, const int64_t* vert_offset,
                        const int64_t* face_offset, int64_t n_objects, int64_t n_verts, int64_t n_faces, double* area_terms,
                        double* volume_terms, void* stream) {
    const int rc = packed_sizes(n_objects, n_verts, n_faces);
    if (rc != SNR_OK) return rc;
    if (n_faces == 0) return SNR_OK;
    if (n_objects == 0 || !verts || !faces || !root || !vert_offset || !face_offset || !area_terms || !volume_terms) return SNR_E_ARG;
    mesh_face_terms_kernel<<<grid_blocks(n_faces), GRID_THREADS, 0, (hipStream_t)stream>>>(
        verts, faces, root, (const long long*)order, (const long long*)vert_offset, (const long long*)face_offset, n_objects, n_verts, n_faces,
        area_terms, volume_terms);
    return snr_check_launch_();
}

int64_t snr_segment_slab_bound(int64_t n_segments, int64_t n_items) {
    if (n_segments < 0 || n_items < 0) return 0;
    return n_segments + n_items / SEGMENT_SLAB;
}

int snr_mesh_segment_sum(const double* area_terms, const double* volume_terms, const int64_t* seg_start, const int64_t* slab_offset,
                         int64_t n_comps, int64_t n_faces, double* partial, int64_t n_slabs, double* area, double* volume, void* stream) {
    const int rc = packed_sizes(0, n_comps, n_faces);
    if (rc != SNR_OK) return rc;
    if (n_slabs < 0) return SNR_E_ARG;
    if (n_comps == 0) return SNR_OK;
    if (n_slabs < snr_segment_slab_bound(n_comps, n_faces)) return SNR_E_WORKSPACE;
    if (n_slabs > 0x7fffffffll) return SNR_E_UNSUPPORTED;
    if (!seg_start || !slab_offset || !partial || !area || !volume || (n_faces && (!area_terms || !volume_terms))) return SNR_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    mesh_slab_sum_kernel<<<(unsigned)n_slabs, GRID_THREADS, 0, st>>>(area_terms, volume_terms, (const long long*)seg_start,
                                                                     (const long long*)slab_offset, n_comps, n_faces, partial);
    mesh_comp_sum_kernel<<<grid_blocks(n_comps * 64), GRID_THREADS, 0, st>>>(partial, (const long long*)slab_offset, n_comps, n_slabs, area,
                                                                             volume);
    return snr_check_launch_();
}

}  // extern "C"
