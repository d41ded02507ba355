// The stretch of a scene iteration between the object poses and the decoder, and between the decoder and the composite, as single launches
// for gfx950 (rules: include/supnerf_hip.h, snr_scene_samples_fwd):
//   * scene_samples_fwd: camera-in-object poses + rois + listed pixels -> every (pixel, object) pair's ray (scene.scene_ray_rows), its box or
//                        sphere bounds and its S samples in the decoder's layout and the composite's (scene.render_scene_batch);
//   * scene_samples_bwd: d(points), d(directions), d(metric depths) -> d(poses), through the bounds; two launches, fixed association;
//   * scene_gather_fwd / bwd: the decoder's object-major outputs <-> the composite's pixel-major rows, (0, white) on pairs that are not hit;
//   * scene_pair_hits, scene_samples_compact_fwd / bwd, scene_gather_compact_fwd / bwd: the same chain with only the pairs that hit handed to
//     the decoder, `capacity` slots per object, a pair's slot its rank among its object's hits (the caller's prefix sum of the flags).
// All HBM-bound.  One workgroup owns PAIRS consecutive pixels of one object: its threads first set the pairs up (one pair each, in double:
// a few dozen flops against S samples of traffic), park what the samples need in LDS, then sweep the samples in memory order.
// The dense and the compact entry points run the same four kernels, scene_samples_fwd / _bwd_kernel and scene_gather_fwd / _bwd_kernel, as
// template <bool COMPACT> instantiations: the routes differ only in which row of the decoder's layout a pair owns (b * Nr + r | b * C + slot),
// which flag array is written (hit | kept) and the compact forward's padding tail; scene_pair_hits_kernel and scene_samples_sum_kernel have
// no twin.
#include "snr_device.hpp"
#include "snr_host.hpp"

namespace snr {

constexpr int PAIRS = 256;        // (pixel, object) pairs per workgroup = threads per workgroup

struct SceneCam { float fx, fy, cx, cy; };

// what one (pixel, object) pair's samples are made from; `hit` false: nothing else is defined
struct PairRay {
    double u[3];           // unit direction in the object frame
    double c[2];           // the pixel's camera direction (c0, c1, 1)
    double inv_n;          // 1 / |R c|
    double near, far;
    int a_near, a_far;     // the axis whose slab gives near / far (-1: sphere bounds)
    bool hit;
};

struct ObjFrame {
    double R[9], t[3];     // cam2obj = [R | t]
    double hd;             // diag / 2
    double half[3];        // box half sizes / (diag / 2): (l, w, h) / diag
    int x0, y0, x1, y1;
    bool live;
};

__device__ __forceinline__ ObjFrame load_object(const float* __restrict__ cam2obj, const float* __restrict__ wlh, const int32_t* __restrict__ rois,
                                                long long b) {
    ObjFrame f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) f.R[3 * i + j] = cam2obj[b * 12 + 4 * i + j];
        f.t[i] = cam2obj[b * 12 + 4 * i + 3];
    }
    const double w = wlh[b * 3], l = wlh[b * 3 + 1], h = wlh[b * 3 + 2];
    const double diag = sqrt(w * w + l * l + h * h);
    f.hd = 0.5 * diag;
    f.half[0] = l / diag; f.half[1] = w / diag; f.half[2] = h / diag;
    f.x0 = rois[b * 4]; f.y0 = rois[b * 4 + 1]; f.x1 = rois[b * 4 + 2]; f.y1 = rois[b * 4 + 3];
    f.live = f.x1 > f.x0 && f.y1 > f.y0;
    return f;
}

// coverage, direction, bounds and the hit decision of one pair
__device__ __forceinline__ PairRay make_pair(const ObjFrame& f, int x, int y, SceneCam k, bool rend_aabb) {
    PairRay p;
    p.hit = false;
    p.a_near = p.a_far = -1;
    if (!(f.live && x >= f.x0 && x < f.x1 && y >= f.y0 && y < f.y1)) return p;
    p.c[0] = ((double)x - (double)k.cx) / (double)k.fx;
    p.c[1] = ((double)y - (double)k.cy) / (double)k.fy;
    double w[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] = p.c[0] * f.R[3 * i] + p.c[1] * f.R[3 * i + 1] + f.R[3 * i + 2];
    p.inv_n = 1.0 / sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) p.u[i] = w[i] * p.inv_n;
    if (!rend_aabb) {      // the sphere around the object: |camera centre| -/+ diag/2, in units of diag/2
        const double dist = sqrt(f.t[0] * f.t[0] + f.t[1] * f.t[1] + f.t[2] * f.t[2]);
        p.near = (dist - f.hd) / f.hd;
        p.far = (dist + f.hd) / f.hd;
        p.hit = p.far > p.near && p.far > 0.0;
        return p;
    }
    double near = -INFINITY, far = INFINITY;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double o = f.t[a] / f.hd;
        if (p.u[a] == 0.0) {       // parallel to the slab: inside it the axis bounds nothing, on or outside it the ray misses
            if (o > -f.half[a] && o < f.half[a]) continue;
            return p;
        }
        const double inv = 1.0 / p.u[a];
        const double ta = (-f.half[a] - o) * inv, tb = (f.half[a] - o) * inv;
        const double lo = fmin(ta, tb), hi = fmax(ta, tb);
        if (lo > near) { near = lo; p.a_near = a; }
        if (hi < far) { far = hi; p.a_far = a; }
    }
    p.near = near; p.far = far;
    p.hit = far > near && far > 0.0;      // (strict: touching an edge or a box behind the camera is a miss)
    return p;
}

// v[a] without a register array indexed at run time (that would live in scratch)
__device__ __forceinline__ double pick3(const double v[3], int a) { return a == 0 ? v[0] : (a == 1 ? v[1] : v[2]); }

// what the sweeps read per pair from LDS
struct PairLds { double u[3], near, far; };

// sample k of a pair that is hit: point, direction and metric depth, each rounded to fp32 once
__device__ __forceinline__ void sample_fwd(const ObjFrame& f, const double o[3], const PairLds& p, int k, const float* __restrict__ jitter, long long ip,
                                           double inv_s, double scale, int shapenet, float px[3], float dv[3], float& z) {
    const double tau = ((double)k + (jitter ? (double)jitter[ip] : 0.0)) * inv_s;
    const double zk = p.near * (1.0 - tau) + p.far * tau;
    const double pt[3] = {(o[0] + zk * p.u[0]) * scale, (o[1] + zk * p.u[1]) * scale, (o[2] + zk * p.u[2]) * scale};
    if (shapenet) {
        px[0] = (float)-pt[1]; px[1] = (float)pt[0]; px[2] = (float)pt[2];
        dv[0] = (float)-p.u[1]; dv[1] = (float)p.u[0]; dv[2] = (float)p.u[2];
    } else {
        px[0] = (float)pt[0]; px[1] = (float)pt[1]; px[2] = (float)pt[2];
        dv[0] = (float)p.u[0]; dv[1] = (float)p.u[1]; dv[2] = (float)p.u[2];
    }
    z = (float)(fabs(zk) * sqrt(p.u[0] * p.u[0] + p.u[1] * p.u[1] + p.u[2] * p.u[2]) * f.hd);
}

// what a pair that is not hit holds: finite inputs for the decoder, depth -1
__device__ __forceinline__ void sample_miss(float px[3], float dv[3], float& z) {
    px[0] = px[1] = px[2] = 0.f;
    dv[0] = dv[1] = 0.f; dv[2] = 1.f;
    z = -1.f;
}

__device__ __forceinline__ void park_pair(PairLds& q, const PairRay& p) {
    q.u[0] = p.u[0]; q.u[1] = p.u[1]; q.u[2] = p.u[2]; q.near = p.near; q.far = p.far;
}

// the slot of a hit pair, -1 when it is not kept: scan is only compared, a value outside [1, C] keeps nothing
__device__ __forceinline__ int slot_of(bool hit, int32_t scan, int C) { return hit && scan >= 1 && scan <= C ? scan - 1 : -1; }

// how many of an object's C slots are taken: its true count, clamped
__device__ __forceinline__ int slots_taken(const int32_t* __restrict__ scan, long long Nr, int Nb, long long b, int C) {
    if (Nr <= 0) return 0;
    const int32_t n = scan[(Nr - 1) * Nb + b];
    return n < 0 ? 0 : (n > C ? C : n);
}

// The slot a thread parks for its pair decides everything the two routes differ in.  Dense: 0 on a hit, -1 otherwise; the pair's row of the
// decoder's layout is b * Nr + r and every row is written, a miss with sample_miss.  COMPACT: slot_of(hit, scan); the row is b * C + slot, only
// kept pairs have one, and the workgroups of an object share out its padding slots.  `flag` is hit (dense) / kept (compact); only dense
// fills `valid`, only compact reads `scan` and fills `pair_of_slot`.
template <bool COMPACT>
__global__ void __launch_bounds__(PAIRS) scene_samples_fwd_kernel(const float* __restrict__ cam2obj, const float* __restrict__ wlh,
                                                                  const int32_t* __restrict__ rois, const int32_t* __restrict__ pixels, SceneCam cam,
                                                                  const float* __restrict__ jitter, long long Nr, int Nb, int S, float adjust_scale,
                                                                  int rend_aabb, int shapenet, const int32_t* __restrict__ scan, int C,
                                                                  float* __restrict__ xyz, float* __restrict__ viewdir, float* __restrict__ z_vals,
                                                                  uint8_t* __restrict__ flag, uint8_t* __restrict__ valid,
                                                                  int32_t* __restrict__ pair_of_slot) {
    __shared__ PairLds prm[PAIRS];
    __shared__ int slots[PAIRS];
    const long long b = blockIdx.y;
    const long long r0 = (long long)blockIdx.x * PAIRS;
    const long long left = Nr - r0;                              // (<= 0: the compact launch with Nr = 0, padding only)
    const int np = (int)(left < 0 ? 0 : (left < PAIRS ? left : PAIRS));
    const long long R = COMPACT ? C : Nr;                        // rows per object of the decoder's layout
    const ObjFrame f = load_object(cam2obj, wlh, rois, b);
    if ((int)threadIdx.x < np) {
        const long long r = r0 + threadIdx.x;
        const int x = pixels[2 * r], y = pixels[2 * r + 1];
        const PairRay p = make_pair(f, x, y, cam, rend_aabb != 0);
        const int slot = COMPACT ? slot_of(p.hit, scan[r * Nb + b], C) : (p.hit ? 0 : -1);
        slots[threadIdx.x] = slot;
        flag[r * Nb + b] = slot >= 0 ? 1 : 0;
        if (slot >= 0) park_pair(prm[threadIdx.x], p);
        if constexpr (COMPACT) {
            if (slot >= 0) pair_of_slot[b * C + slot] = (int32_t)r;
        } else if (valid && b == 0) {       // some object is hit: the workgroups of object 0 look at the others too
            bool any = p.hit;
            for (long long b2 = 1; b2 < Nb && !any; ++b2) any = make_pair(load_object(cam2obj, wlh, rois, b2), x, y, cam, rend_aabb != 0).hit;
            valid[r] = any ? 1 : 0;
        }
    }
    __syncthreads();
    const double o[3] = {f.t[0] / f.hd, f.t[1] / f.hd, f.t[2] / f.hd};
    const double scale = (double)adjust_scale, inv_s = 1.0 / (double)S;
    const long long n = (long long)np * S;
    for (long long e = threadIdx.x; e < n; e += PAIRS) {
        const int q = (int)(e / S), k = (int)(e - (long long)q * S);
        const long long r = r0 + q;
        const long long ip = (r * Nb + b) * S + k;              // pixel-major: the composite's (and the jitter's)
        const int slot = slots[q];
        float px[3], dv[3], z;
        if (slot >= 0) {
            sample_fwd(f, o, prm[q], k, jitter, ip, inv_s, scale, shapenet, px, dv, z);
        } else {
            sample_miss(px, dv, z);
            if (COMPACT) { z_vals[ip] = z; continue; }          // no row to write
        }
        const long long io = ((b * R + (COMPACT ? slot : r)) * S + k) * 3;            // object-major: the decoder's layout
#pragma unroll
        for (int c = 0; c < 3; ++c) { xyz[io + c] = px[c]; viewdir[io + c] = dv[c]; }
        z_vals[ip] = z;
    }
    if constexpr (COMPACT) {     // padding: slots taken .. C-1 of this object, an equal run of them per workgroup
        const int taken = slots_taken(scan, Nr, Nb, b, C);
        const int run = (C + (int)gridDim.x - 1) / (int)gridDim.x;
        const long long lo0 = (long long)blockIdx.x * run, hi0 = lo0 + run;
        const int lo = (int)(lo0 < taken ? taken : (lo0 > C ? C : lo0)), hi = (int)(hi0 > C ? C : hi0);
        if (hi <= lo) return;
        for (int sl = lo + (int)threadIdx.x; sl < hi; sl += PAIRS) pair_of_slot[b * C + sl] = -1;
        float px[3], dv[3], z;
        sample_miss(px, dv, z);
        const long long m = (long long)(hi - lo) * S;
        for (long long e = threadIdx.x; e < m; e += PAIRS) {
            const long long io = ((b * C + lo) * S + e) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) { xyz[io + c] = px[c]; viewdir[io + c] = dv[c]; }
        }
    }
}

// Stage 1 of the backward: the 12 sums of one object's slice of PAIRS pixels.  Every sample's contribution to d(cam2obj) is LINEAR in its
// upstream gradients with coefficients of its pair, so a thread applies the pair's map to each of its samples and keeps 12 double sums of its
// own: no reduction per pair.  The sums meet in LDS in thread order (pose_rays_bwd_kernel's scheme) and leave as one row of `partial`.
struct PairBwd { double u[3], c[2], inv_n, near, far, gn[2], gf[2]; int a_near, a_far; };

__device__ __forceinline__ void park_pair_bwd(PairBwd& q, const PairRay& p) {
    q.u[0] = p.u[0]; q.u[1] = p.u[1]; q.u[2] = p.u[2]; q.c[0] = p.c[0]; q.c[1] = p.c[1];
    q.inv_n = p.inv_n; q.near = p.near; q.far = p.far; q.a_near = p.a_near; q.a_far = p.a_far;
    // near = (plane - o_a) / u_a on its axis a: d near / d o_a = -1 / u_a, d near / d u_a = -near / u_a (far likewise).  An axis with
    // u_a == 0 is never the one that bounds a hit, so it adds nothing.
    const double un = pick3(p.u, p.a_near), uf = pick3(p.u, p.a_far);
    if (p.a_near >= 0) { q.gn[0] = -1.0 / un; q.gn[1] = -p.near / un; } else { q.gn[0] = q.gn[1] = 0.0; }
    if (p.a_far >= 0) { q.gf[0] = -1.0 / uf; q.gf[1] = -p.far / uf; } else { q.gf[0] = q.gf[1] = 0.0; }
}

// sample k of a pair that is hit, added to the thread's 12 sums; io: its row in d_xyz / d_viewdir, ip: in d_z and the jitter
__device__ __forceinline__ void sample_bwd(const ObjFrame& f, const PairBwd& p, int k, const float* __restrict__ jitter, long long io, long long ip,
                                           double inv_s, double scale, int rend_aabb, int shapenet, double dist, const float* __restrict__ d_xyz,
                                           const float* __restrict__ d_viewdir, const float* __restrict__ d_z, double gR[9], double gt[3]) {
    const double tau = ((double)k + (jitter ? (double)jitter[ip] : 0.0)) * inv_s;
    const double zk = p.near * (1.0 - tau) + p.far * tau;
    double G[3] = {0., 0., 0.}, gu[3] = {0., 0., 0.};
    if (d_xyz) {             // gradient of (o + z u): the frame swap (x,y,z) -> (-y,x,z) undone, times the scale
        const double g0 = d_xyz[io], g1 = d_xyz[io + 1], g2 = d_xyz[io + 2];
        if (shapenet) { G[0] = g1 * scale; G[1] = -g0 * scale; G[2] = g2 * scale; }
        else { G[0] = g0 * scale; G[1] = g1 * scale; G[2] = g2 * scale; }
    }
    if (d_viewdir) {
        const double g0 = d_viewdir[io], g1 = d_viewdir[io + 1], g2 = d_viewdir[io + 2];
        if (shapenet) { gu[0] = g1; gu[1] = -g0; gu[2] = g2; } else { gu[0] = g0; gu[1] = g1; gu[2] = g2; }
    }
    // the metric depth |z| |u| diag/2: its gradient to u lies along u and the normalisation below removes it
    double gz = G[0] * p.u[0] + G[1] * p.u[1] + G[2] * p.u[2];
    if (d_z) gz += (double)d_z[ip] * (zk > 0.0 ? f.hd : (zk < 0.0 ? -f.hd : 0.0));
    const double g_near = gz * (1.0 - tau), g_far = gz * tau;
    double go[3] = {G[0], G[1], G[2]};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        gu[a] += zk * G[a];
        if (a == p.a_near) { go[a] += g_near * p.gn[0]; gu[a] += g_near * p.gn[1]; }
        if (a == p.a_far) { go[a] += g_far * p.gf[0]; gu[a] += g_far * p.gf[1]; }
    }
    // u = w / |w|, w = R c: the part of gu along u is projected off
    const double dot = p.u[0] * gu[0] + p.u[1] * gu[1] + p.u[2] * gu[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double gw = (gu[i] - p.u[i] * dot) * p.inv_n;
        gR[3 * i] += gw * p.c[0]; gR[3 * i + 1] += gw * p.c[1]; gR[3 * i + 2] += gw;
        // o = t / (diag/2); the sphere bounds move with |t|
        double g = go[i] / f.hd;
        if (!rend_aabb) g += (g_near + g_far) * f.t[i] / (dist * f.hd);
        gt[i] += g;
    }
}

// the threads' 12 sums meet in LDS in thread order and leave as the workgroup's row of `partial`
__device__ __forceinline__ void meet_slice(double (&part)[12][PAIRS], double (&part2)[12][16], const double gR[9], const double gt[3],
                                           double* __restrict__ row) {
#pragma unroll
    for (int i = 0; i < 9; ++i) part[i][threadIdx.x] = gR[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) part[9 + i][threadIdx.x] = gt[i];
    __syncthreads();
    if (threadIdx.x < 12 * 16) {
        const int q = threadIdx.x >> 4, seg = threadIdx.x & 15;
        double sum = 0.;
        for (int k = 0; k < PAIRS / 16; ++k) sum += part[q][seg * (PAIRS / 16) + k];
        part2[q][seg] = sum;
    }
    __syncthreads();
    if (threadIdx.x < 12) {
        double sum = 0.;
#pragma unroll
        for (int k = 0; k < 16; ++k) sum += part2[threadIdx.x][k];
        row[threadIdx.x] = sum;
    }
}

// scene_samples_fwd_kernel's slot policy on the way back: d_xyz and d_viewdir are read at row b * Nr + r (dense) or b * C + slot (COMPACT);
// the pairs of a slice, the sweep and the meeting order are one and the same, so the two routes add the same numbers in the same order
template <bool COMPACT>
__global__ void __launch_bounds__(PAIRS) scene_samples_bwd_kernel(const float* __restrict__ cam2obj, const float* __restrict__ wlh,
                                                                  const int32_t* __restrict__ rois, const int32_t* __restrict__ pixels, SceneCam cam,
                                                                  const float* __restrict__ jitter, long long Nr, int Nb, int S, float adjust_scale,
                                                                  int rend_aabb, int shapenet, const int32_t* __restrict__ scan, int C,
                                                                  const float* __restrict__ d_xyz, const float* __restrict__ d_viewdir,
                                                                  const float* __restrict__ d_z, double* __restrict__ partial) {
    __shared__ PairBwd prm[PAIRS];
    __shared__ int slots[PAIRS];
    __shared__ double part[12][PAIRS];
    __shared__ double part2[12][16];
    const long long b = blockIdx.y;
    const long long r0 = (long long)blockIdx.x * PAIRS;
    const int np = (int)(Nr - r0 < PAIRS ? Nr - r0 : PAIRS);
    const long long R = COMPACT ? C : Nr;
    const ObjFrame f = load_object(cam2obj, wlh, rois, b);
    if ((int)threadIdx.x < np) {
        const long long r = r0 + threadIdx.x;
        const PairRay p = make_pair(f, pixels[2 * r], pixels[2 * r + 1], cam, rend_aabb != 0);
        const int slot = COMPACT ? slot_of(p.hit, scan[r * Nb + b], C) : (p.hit ? 0 : -1);
        slots[threadIdx.x] = slot;
        if (slot >= 0) park_pair_bwd(prm[threadIdx.x], p);
    }
    __syncthreads();
    const double scale = (double)adjust_scale, inv_s = 1.0 / (double)S;
    double dist = 1.0;
    if (!rend_aabb) dist = sqrt(f.t[0] * f.t[0] + f.t[1] * f.t[1] + f.t[2] * f.t[2]);
    double gR[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.}, gt[3] = {0., 0., 0.};
    const long long n = (long long)np * S;
    for (long long e = threadIdx.x; e < n; e += PAIRS) {
        const int q = (int)(e / S), k = (int)(e - (long long)q * S);
        const int slot = slots[q];
        if (slot < 0) continue;                                  // not hit, or dropped: exact zeros
        const long long r = r0 + q;
        sample_bwd(f, prm[q], k, jitter, ((b * R + (COMPACT ? slot : r)) * S + k) * 3, (r * Nb + b) * S + k, inv_s, scale, rend_aabb, shapenet, dist,
                   d_xyz, d_viewdir, d_z, gR, gt);
    }
    meet_slice(part, part2, gR, gt, partial + (b * gridDim.x + blockIdx.x) * 12);
}

// Stage 2: the slices of every object added in slice order; element (i, j) of d_cam2obj (Nb,3,4) = [dL/dR | dL/dt]
__global__ void __launch_bounds__(64) scene_samples_sum_kernel(const double* __restrict__ partial, long long slices, float* __restrict__ d_cam2obj) {
    const long long b = blockIdx.x;
    if (threadIdx.x >= 12) return;
    const int i = threadIdx.x / 4, j = threadIdx.x % 4;
    const int q = j < 3 ? 3 * i + j : 9 + i;
    double sum = 0.;
    for (long long s = 0; s < slices; ++s) sum += partial[(b * slices + s) * 12 + q];
    d_cam2obj[b * 12 + threadIdx.x] = (float)sum;
}

// pixel-major rows of the decoder's object-major outputs, (0, white) where the pair has no row: dense, row b * Nr + r where `flag` = hit says
// so; COMPACT, row b * C + slot with the slot from `flag` = kept and scan
template <bool COMPACT>
__global__ void __launch_bounds__(256) scene_gather_fwd_kernel(const float* __restrict__ sigmas, const float* __restrict__ rgbs,
                                                               const int32_t* __restrict__ scan, const uint8_t* __restrict__ flag, long long Nr,
                                                               int Nb, int S, int C, float* __restrict__ sig_out, float* __restrict__ rgb_out) {
    const long long n = Nr * Nb * S;
    for (long long e = blockIdx.x * 256ll + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const long long pair = e / S;
        const int k = (int)(e - pair * S);
        const long long r = pair / Nb, b = pair - r * Nb;
        const int slot = COMPACT ? slot_of(flag[pair] != 0, scan[pair], C) : (flag[pair] != 0 ? 0 : -1);
        const bool h = slot >= 0;
        const long long src = (COMPACT ? b * C + (h ? slot : 0) : b * Nr + r) * S + k;
        if (sig_out) sig_out[e] = h ? sigmas[src] : 0.f;
        if (rgb_out) {
#pragma unroll
            for (int c = 0; c < 3; ++c) rgb_out[3 * e + c] = h ? rgbs[3 * src + c] : 1.f;
        }
    }
}

// the inverse scatter in the destination's order, Nb * R rows: dense (R = Nr), row b * Nr + r takes pixel r where hit says so; COMPACT
// (R = C), slot (b, s) takes pixel pair_of_slot[b][s], range-checked; exact zeros on every other row
template <bool COMPACT>
__global__ void __launch_bounds__(256) scene_gather_bwd_kernel(const float* __restrict__ d_sig_rows, const float* __restrict__ d_rgb_rows,
                                                               const uint8_t* __restrict__ hit, const int32_t* __restrict__ pair_of_slot,
                                                               long long Nr, int Nb, int S, int C, float* __restrict__ d_sigmas,
                                                               float* __restrict__ d_rgbs) {
    const long long R = COMPACT ? C : Nr;
    const long long n = (long long)Nb * R * S;
    for (long long e = blockIdx.x * 256ll + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const long long row = e / S;
        const int k = (int)(e - row * S);
        const long long b = row / R;
        long long r;
        bool h;
        if constexpr (COMPACT) { r = pair_of_slot[row]; h = r >= 0 && r < Nr; if (!h) r = 0; }
        else { r = row - b * R; h = hit[r * Nb + b] != 0; }
        const long long src = (r * Nb + b) * S + k;
        if (d_sigmas) d_sigmas[e] = h ? d_sig_rows[src] : 0.f;
        if (d_rgbs) {
#pragma unroll
            for (int c = 0; c < 3; ++c) d_rgbs[3 * e + c] = h ? d_rgb_rows[3 * src + c] : 0.f;
        }
    }
}

// the hit flags alone: what scene_samples_fwd_kernel decides, for the compact route's prefix sum
__global__ void __launch_bounds__(PAIRS) scene_pair_hits_kernel(const float* __restrict__ cam2obj, const float* __restrict__ wlh,
                                                                const int32_t* __restrict__ rois, const int32_t* __restrict__ pixels, SceneCam cam,
                                                                long long Nr, int Nb, int rend_aabb, uint8_t* __restrict__ hit) {
    const long long b = blockIdx.y;
    const long long r = (long long)blockIdx.x * PAIRS + threadIdx.x;
    if (r >= Nr) return;
    const ObjFrame f = load_object(cam2obj, wlh, rois, b);
    hit[r * Nb + b] = make_pair(f, pixels[2 * r], pixels[2 * r + 1], cam, rend_aabb != 0).hit ? 1 : 0;
}

inline long long scene_slices(long long Nr) { return (Nr + PAIRS - 1) / PAIRS; }
// sizes the kernels' 64-bit indices and grids take: Nb objects in gridDim.y, Nr * Nb * S * 3 elements
inline bool scene_sizes_ok(long long Nr, long long Nb, int S) {
    return Nr >= 0 && Nb >= 1 && Nb <= 65535 && S >= 1 && Nr <= (1ll << 40) / (Nb * (long long)S) && scene_slices(Nr) <= 0x7fffffffll;
}
// a capacity the compact kernels take: whole 32-point tiles per object for every S, Nb * C * S * 3 elements within the same limit
inline bool scene_capacity_ok(long long C, long long Nb, int S) { return C >= 1 && C <= 0x7fffffffll && C % 32 == 0 && scene_sizes_ok(C, Nb, S); }

}  // namespace snr

using namespace snr;

// The backward's two launches, after an entry point's own argument checks: the workspace, every slice's 12 sums, then every object's slices
// added in slice order.
template <bool COMPACT>
static int scene_samples_bwd_run(const float* cam2obj, const float* wlh, const int32_t* rois, const int32_t* pixels, SceneCam cam, const float* jitter,
                                 int64_t n_pixels, int64_t n_objects, int n_samples, float adjust_scale, int rend_aabb, int shapenet,
                                 const int32_t* scan, int C, const float* d_xyz, const float* d_viewdir, const float* d_z, float* d_cam2obj, void* ws,
                                 size_t ws_bytes, hipStream_t stream) {
    if (((uintptr_t)ws & 7) != 0) return SNR_E_ARG;
    if (ws_bytes < snr_scene_samples_bwd_ws_bytes(n_pixels, n_objects)) return SNR_E_WORKSPACE;
    const long long slices = scene_slices(n_pixels);
    scene_samples_bwd_kernel<COMPACT><<<dim3((unsigned)slices, (unsigned)n_objects), PAIRS, 0, stream>>>(
        cam2obj, wlh, rois, pixels, cam, jitter, n_pixels, (int)n_objects, n_samples, adjust_scale, rend_aabb, shapenet, scan, C, d_xyz, d_viewdir, d_z,
        (double*)ws);
    const int rc = snr_check_launch_();
    if (rc != SNR_OK) return rc;
    scene_samples_sum_kernel<<<(unsigned)n_objects, 64, 0, stream>>>((const double*)ws, slices, d_cam2obj);
    return snr_check_launch_();
}

extern "C" {

int snr_scene_samples_fwd(const float* cam2obj, const float* wlh, const int32_t* rois, const int32_t* pixels, float fx, float fy, float cx, float cy,
                          const float* jitter, int64_t n_pixels, int64_t n_objects, int n_samples, float adjust_scale, int rend_aabb,
                          int shapenet_obj_cood, float* xyz, float* viewdir, float* z_vals, uint8_t* hit, uint8_t* valid, void* stream) {
    if (n_pixels == 0) return SNR_OK;
    if (!scene_sizes_ok(n_pixels, n_objects, n_samples)) return SNR_E_ARG;
    if (!cam2obj || !wlh || !rois || !pixels || !xyz || !viewdir || !z_vals || !hit) return SNR_E_ARG;
    const SceneCam cam = {fx, fy, cx, cy};
    scene_samples_fwd_kernel<false><<<dim3((unsigned)scene_slices(n_pixels), (unsigned)n_objects), PAIRS, 0, (hipStream_t)stream>>>(
        cam2obj, wlh, rois, pixels, cam, jitter, n_pixels, (int)n_objects, n_samples, adjust_scale, rend_aabb, shapenet_obj_cood, nullptr, 0, xyz,
        viewdir, z_vals, hit, valid, nullptr);
    return snr_check_launch_();
}

size_t snr_scene_samples_bwd_ws_bytes(int64_t n_pixels, int64_t n_objects) {
    if (n_pixels <= 0 || n_objects <= 0) return 0;
    return (size_t)scene_slices(n_pixels) * (size_t)n_objects * 12 * sizeof(double);
}

int snr_scene_samples_bwd(const float* cam2obj, const float* wlh, const int32_t* rois, const int32_t* pixels, float fx, float fy, float cx, float cy,
                          const float* jitter, int64_t n_pixels, int64_t n_objects, int n_samples, float adjust_scale, int rend_aabb,
                          int shapenet_obj_cood, const float* d_xyz, const float* d_viewdir, const float* d_z, float* d_cam2obj, void* ws,
                          size_t ws_bytes, void* stream) {
    if (n_pixels == 0) return SNR_OK;
    if (!scene_sizes_ok(n_pixels, n_objects, n_samples)) return SNR_E_ARG;
    if (!cam2obj || !wlh || !rois || !pixels || !d_cam2obj || !ws) return SNR_E_ARG;
    return scene_samples_bwd_run<false>(cam2obj, wlh, rois, pixels, {fx, fy, cx, cy}, jitter, n_pixels, n_objects, n_samples, adjust_scale, rend_aabb,
                                        shapenet_obj_cood, nullptr, 0, d_xyz, d_viewdir, d_z, d_cam2obj, ws, ws_bytes, (hipStream_t)stream);
}

static unsigned gather_grid(long long n) {
    long long g = (n + 255) / 256;
    return (unsigned)(g > 65536 ? 65536 : (g < 1 ? 1 : g));
}

int snr_scene_gather_fwd(const float* sigmas, const float* rgbs, const uint8_t* hit, int64_t n_pixels, int64_t n_objects, int n_samples,
                         float* sigma_rows, float* rgb_rows, void* stream) {
    if (n_pixels == 0) return SNR_OK;
    if (!scene_sizes_ok(n_pixels, n_objects, n_samples)) return SNR_E_ARG;
    if (!hit || (sigma_rows && !sigmas) || (rgb_rows && !rgbs) || (!sigma_rows && !rgb_rows)) return SNR_E_ARG;
    scene_gather_fwd_kernel<false><<<gather_grid(n_pixels * n_objects * n_samples), 256, 0, (hipStream_t)stream>>>(
        sigmas, rgbs, nullptr, hit, n_pixels, (int)n_objects, n_samples, 0, sigma_rows, rgb_rows);
    return snr_check_launch_();
}

int snr_scene_gather_bwd(const float* d_sigma_rows, const float* d_rgb_rows, const uint8_t* hit, int64_t n_pixels, int64_t n_objects, int n_samples,
                         float* d_sigmas, float* d_rgbs, void* stream) {
    if (n_pixels == 0) return SNR_OK;
    if (!scene_sizes_ok(n_pixels, n_objects, n_samples)) return SNR_E_ARG;
    if (!hit || (d_sigmas && !d_sigma_rows) || (d_rgbs && !d_rgb_rows) || (!d_sigmas && !d_rgbs)) return SNR_E_ARG;
    scene_gather_bwd_kernel<false><<<gather_grid(n_pixels * n_objects * n_samples), 256, 0, (hipStream_t)stream>>>(
        d_sigma_rows, d_rgb_rows, hit, nullptr, n_pixels, (int)n_objects, n_samples, 0, d_sigmas, d_rgbs);
    return snr_check_launch_();
}

int snr_scene_pair_hits(const float* cam2obj, const float* wlh, const int32_t* rois, const int32_t* pixels, float fx, float fy, float cx, float cy,
                        int64_t n_pixels, int64_t n_objects, int rend_aabb, uint8_t* hit, void* stream) {
    if (n_pixels == 0) return SNR_OK;
    if (!scene_sizes_ok(n_pixels, n_objects, 1)) return SNR_E_ARG;
    if (!cam2obj || !wlh || !rois || !pixels || !hit) return SNR_E_ARG;
    const SceneCam cam = {fx, fy, cx, cy};
    scene_pair_hits_kernel<<<dim3((unsigned)scene_slices(n_pixels), (unsigned)n_objects), PAIRS, 0, (hipStream_t)stream>>>(
        cam2obj, wlh, rois, pixels, cam, n_pixels, (int)n_objects, rend_aabb, hit);
    return snr_check_launch_();
}

int snr_scene_samples_compact_fwd(const float* cam2obj, const float* wlh, const int32_t* rois, const int32_t* pixels, float fx, float fy, float cx,
                                  float cy, const float* jitter, int64_t n_pixels, int64_t n_objects, int n_samples, float adjust_scale,
                                  int rend_aabb, int shapenet_obj_cood, const int32_t* hit_scan, int64_t capacity, float* xyz, float* viewdir,
                                  float* z_vals, uint8_t* kept, int32_t* pair_of_slot, void* stream) {
    if (!scene_sizes_ok(n_pixels, n_objects, n_samples) || !scene_capacity_ok(capacity, n_objects, n_samples)) return SNR_E_ARG;
    if (!cam2obj || !wlh || !rois || !xyz || !viewdir || !pair_of_slot) return SNR_E_ARG;
    if (n_pixels > 0 && (!pixels || !hit_scan || !z_vals || !kept)) return SNR_E_ARG;
    const SceneCam cam = {fx, fy, cx, cy};
    const long long slices = scene_slices(n_pixels);
    scene_samples_fwd_kernel<true><<<dim3((unsigned)(slices < 1 ? 1 : slices), (unsigned)n_objects), PAIRS, 0, (hipStream_t)stream>>>(
        cam2obj, wlh, rois, pixels, cam, jitter, n_pixels, (int)n_objects, n_samples, adjust_scale, rend_aabb, shapenet_obj_cood, hit_scan,
        (int)capacity, xyz, viewdir, z_vals, kept, nullptr, pair_of_slot);
    return snr_check_launch_();
}

int snr_scene_samples_compact_bwd(const float* cam2obj, const float* wlh, const int32_t* rois, const int32_t* pixels, float fx, float fy, float cx,
                                  float cy, const float* jitter, int64_t n_pixels, int64_t n_objects, int n_samples, float adjust_scale,
                                  int rend_aabb, int shapenet_obj_cood, const int32_t* hit_scan, int64_t capacity, const float* d_xyz,
                                  const float* d_viewdir, const float* d_z, float* d_cam2obj, void* ws, size_t ws_bytes, void* stream) {
    if (!scene_sizes_ok(n_pixels, n_objects, n_samples) || !scene_capacity_ok(capacity, n_objects, n_samples)) return SNR_E_ARG;
    if (n_pixels == 0) return SNR_OK;
    if (!cam2obj || !wlh || !rois || !pixels || !hit_scan || !d_cam2obj || !ws) return SNR_E_ARG;
    return scene_samples_bwd_run<true>(cam2obj, wlh, rois, pixels, {fx, fy, cx, cy}, jitter, n_pixels, n_objects, n_samples, adjust_scale, rend_aabb,
                                       shapenet_obj_cood, hit_scan, (int)capacity, d_xyz, d_viewdir, d_z, d_cam2obj, ws, ws_bytes, (hipStream_t)stream);
}

int snr_scene_gather_compact_fwd(const float* sigmas, const float* rgbs, const int32_t* hit_scan, const uint8_t* kept, int64_t n_pixels,
                                 int64_t n_objects, int n_samples, int64_t capacity, float* sigma_rows, float* rgb_rows, void* stream) {
    if (!scene_sizes_ok(n_pixels, n_objects, n_samples) || !scene_capacity_ok(capacity, n_objects, n_samples)) return SNR_E_ARG;
    if (n_pixels == 0) return SNR_OK;
    if (!hit_scan || !kept || (sigma_rows && !sigmas) || (rgb_rows && !rgbs) || (!sigma_rows && !rgb_rows)) return SNR_E_ARG;
    scene_gather_fwd_kernel<true><<<gather_grid(n_pixels * n_objects * n_samples), 256, 0, (hipStream_t)stream>>>(
        sigmas, rgbs, hit_scan, kept, n_pixels, (int)n_objects, n_samples, (int)capacity, sigma_rows, rgb_rows);
    return snr_check_launch_();
}

int snr_scene_gather_compact_bwd(const float* d_sigma_rows, const float* d_rgb_rows, const int32_t* pair_of_slot, int64_t n_pixels, int64_t n_objects,
                                 int n_samples, int64_t capacity, float* d_sigmas, float* d_rgbs, void* stream) {
    if (!scene_sizes_ok(n_pixels, n_objects, n_samples) || !scene_capacity_ok(capacity, n_objects, n_samples)) return SNR_E_ARG;
    if (!pair_of_slot || (!d_sigmas && !d_rgbs)) return SNR_E_ARG;
    if (n_pixels > 0 && ((d_sigmas && !d_sigma_rows) || (d_rgbs && !d_rgb_rows))) return SNR_E_ARG;
    scene_gather_bwd_kernel<true><<<gather_grid(n_objects * capacity * n_samples), 256, 0, (hipStream_t)stream>>>(
        d_sigma_rows, d_rgb_rows, nullptr, pair_of_slot, n_pixels, (int)n_objects, n_samples, (int)capacity, d_sigmas, d_rgbs);
    return snr_check_launch_();
}

}  // extern "C"
