// The depth merge of a pixel's lists, stated once for the scene composite (snr_aux.hip: scene_general_kernel) and its backward
// (snr_scene_bwd.hip: scene_bwd_kernel): the backward is correct only while its ranks equal the forward's.
// `run` > 0: the pixel's n samples are n/run lists of `run` samples each, every list ascending in depth (one object's samples along its
// ray; a list of an object that does not cover the pixel is all -1).  Then a sample's rank is its position in its own list plus, for every
// other list, the number of smaller depths there -- two halving searches per list, O(n log(run) Nb) LDS reads per pixel instead of the n^2
// of the generic rank sort.  The lists are CHECKED to be ascending; a pixel whose lists are not takes the generic path.
#pragma once

namespace snr {

// # entries of the ascending list zr[0..len) that are < v (UPPER: <= v)
template <bool UPPER>
__device__ __forceinline__ int run_bound(const float* zr, int len, float v) {
    int lo = 0;
    while (len > 0) {
        const int half = len >> 1;
        const float m = zr[lo + half];
        const bool go = UPPER ? (m <= v) : (m < v);
        lo = go ? lo + half + 1 : lo;
        len = go ? len - half - 1 : half;
    }
    return lo;
}

// wave-uniform: the wave's depth row zs[0..n) is whole lists of `run` > 1 depths and every list ascends
__device__ __forceinline__ bool scene_lists_ascend(const float* zs, int n, int run, int lane) {
    bool ascend = false;
    if (run > 1 && n % run == 0) {
        bool sorted = true;
        for (int i = lane; i < n; i += 64) sorted = sorted && ((i % run) == run - 1 || zs[i] <= zs[i + 1]);
        ascend = __all(sorted);
    }
    return ascend;
}

// Sample i (depth zi) among the n_runs verified lists: lt depths are smaller; of the equal ones eb come before it in memory order and ea
// after.  Its sorted slot is lt + eb; a group of equal depths hands its data to slot lt from the member with ea == 0.
struct SceneRank { int lt, eb, ea; };

__device__ __forceinline__ SceneRank scene_list_rank(const float* zs, int n_runs, int run, int i, float zi) {
    const int r = i / run, p = i - r * run;
    SceneRank k = {0, 0, 0};
    for (int q = 0; q < n_runs; ++q) {
        const float* zr = zs + q * run;
        const int lb = run_bound<false>(zr, run, zi);
        const bool has_eq = lb < run && zr[lb] == zi;
        const int ub = has_eq ? lb + 1 + run_bound<true>(zr + lb + 1, run - lb - 1, zi) : lb;
        k.lt += lb;
        if (q < r) k.eb += ub - lb;
        else if (q > r) k.ea += ub - lb;
        else { k.eb += p - lb; k.ea += ub - p - 1; }
    }
    return k;
}

}  // namespace snr
