// bbx_stats.h -- device code shared by bbx_match.hip, bbx_shapes.hip, bbx_psfbuild.hip and bbx_aper.hip: clipped statistics of a
// (y, x)-sorted source list per sub-image tile and of the frame (one workgroup of STATS_BLOCK threads per segment: count,
// strided selection in list order, LDS sort, sigma clipping on the sorted sample, float64 sums in a fixed order).
// bbx_aper.hip takes the clip alone (stats_clip<256> on its annulus sample).
#pragma once
#include "bbx_common.h"

#define STATS_BLOCK   1024
#define STATS_WAVES   (STATS_BLOCK / 64)

// ---- segments of a list sorted by y ------------------------------------------------------------------------------------
__device__ __forceinline__ int match_lower_bound(const int32_t* __restrict__ ys, int n, int y) {     // first i with ys[i] >= y
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (ys[mid] < y) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct stats_seg { int i0, i1, y0, y1, x0, x1, stride; };            // list range, tile rectangle, selection stride

// segment seg of nsy * nsx + 1: a tile of size x size pixels (the list is sorted by y: the tile's rows are one range), or,
// last, the whole frame; stride 1
__device__ __forceinline__ stats_seg stats_segment(int seg, int size, int nsy, int nsx, const int32_t* __restrict__ ys, int n) {
    stats_seg sg;
    if (seg < nsy * nsx) {
        const int ty = seg / nsx, tx = seg - ty * nsx;
        sg.y0 = ty * size; sg.y1 = sg.y0 + size; sg.x0 = tx * size; sg.x1 = sg.x0 + size;
        sg.i0 = match_lower_bound(ys, n, sg.y0);
        sg.i1 = match_lower_bound(ys, n, sg.y1);
    } else {
        sg.y0 = sg.x0 = INT32_MIN; sg.y1 = sg.x1 = INT32_MAX;
        sg.i0 = 0; sg.i1 = n;
    }
    sg.stride = 1;
    return sg;
}

// One walk over the segment's part of the list in list order: every wave takes a contiguous share, 64 sources at a time.
// it.load(i, sg) says whether source i qualifies for the segment (and may keep what it read).  COUNT: -> the wave's number
// of qualifying sources.  Else: the qualifying source of rank r (list order; [base] = those in the shares before this wave's)
// with r % stride == 0 is handed to it.put(i, r / stride), r / stride < BBX_MATCH_CAP
template <bool COUNT, class Item>
__device__ __forceinline__ int stats_walk(const stats_seg& sg, int base, Item& it) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int len = sg.i1 - sg.i0;
    const int share = ((len + STATS_WAVES - 1) / STATS_WAVES + 63) / 64 * 64;
    const long long b0 = (long long)sg.i0 + (long long)wave * share;
    const int beg = (int)(b0 < sg.i1 ? b0 : sg.i1), end = (int)(b0 + share < sg.i1 ? b0 + share : sg.i1);
    int run = base;
    for (int b = beg; b < end; b += 64) {
        const int i = b + lane;
        const bool q = i < end && it.load(i, sg);
        const unsigned long long mask = __ballot(q);
        if (!COUNT && q) {
            const int rank = run + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
            const int pos = rank / sg.stride;
            if (pos * sg.stride == rank && pos < BBX_MATCH_CAP) it.put(i, pos);
        }
        run += __popcll(mask);
    }
    return run - base;
}

// the segment's number of qualifying sources n -> every thread; sets sg.stride so that at most BBX_MATCH_CAP enter, base = the
// qualifying sources in the shares before this thread's wave.  cnt[STATS_WAVES]: LDS
template <class Item>
__device__ __forceinline__ int stats_count(stats_seg& sg, Item& it, int* cnt, int& base) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int mine = stats_walk<true>(sg, 0, it);
    if (lane == 0) cnt[wave] = mine;
    __syncthreads();
    int n = 0;
    base = 0;
#pragma unroll
    for (int w = 0; w < STATS_WAVES; w++) { if (w < wave) base += cnt[w]; n += cnt[w]; }
    sg.stride = n > BBX_MATCH_CAP ? (n + BBX_MATCH_CAP - 1) / BBX_MATCH_CAP : 1;
    return n;
}

// vals[0..m) -> sorted (lds_sort over the next power of two, padded with +inf), then box_stats: 3 sigma about the exact
// median, spread = population std, at most 5 rounds, stop when nothing is clipped.  On the sorted sample a clipped set is a
// range [lo, hi).  -> n, median, mean, std (every thread), and the range's end values.  By a workgroup of BLOCK threads;
// red[2][2][BLOCK / 64] and ph: wg_sum_tree's
template <int BLOCK>
__device__ __forceinline__ void stats_clip(float* vals, int m, double* red, int& ph, double out[4], float& vlo, float& vhi) {
    const int tid = threadIdx.x;
    int P = 2;
    while (P < m) P <<= 1;
    for (int i = m + tid; i < P; i += BLOCK) vals[i] = __builtin_inff();
    __syncthreads();
    lds_sort<BLOCK>(vals, P);
    int lo = 0, hi = m;
    double med = 0.0, mean = 0.0, std = 0.0;
    for (int round = 0; round <= 5; round++) {                       // rounds 0..4 clip; the last pass only takes the statistics
        const int n = hi - lo;
        if (n == 0) break;
        med = (n & 1) ? (double)vals[lo + n / 2] : ((double)vals[lo + n / 2 - 1] + (double)vals[lo + n / 2]) / 2.0;
        double s[2] = {0.0, 0.0};
        for (int i = lo + tid; i < hi; i += BLOCK) s[0] += (double)vals[i];
        wg_sum_tree<BLOCK / 64>(s, red, ph);
        mean = s[0] / (double)n;
        double ss[2] = {0.0, 0.0};
        for (int i = lo + tid; i < hi; i += BLOCK) { const double d = mean - (double)vals[i]; ss[0] += d * d; }
        wg_sum_tree<BLOCK / 64>(ss, red, ph);
        std = sqrt(ss[0] / (double)n);
        if (round == 5) break;
        const double L = med - 3.0 * std, H = med + 3.0 * std;
        double nc[2] = {0.0, 0.0};                                   // clipped below, above
        for (int i = lo + tid; i < hi; i += BLOCK) {
            const double v = (double)vals[i];
            if (!(v >= L)) nc[0] += 1.0;
            else if (!(v <= H)) nc[1] += 1.0;
        }
        wg_sum_tree<BLOCK / 64>(nc, red, ph);
        if (nc[0] == 0.0 && nc[1] == 0.0) break;
        lo += (int)nc[0]; hi -= (int)nc[1];
    }
    const int n = hi - lo;
    const double nan = __builtin_nan("");
    out[0] = (double)n;
    out[1] = n ? med : nan; out[2] = n ? mean : nan; out[3] = n ? std : nan;
    vlo = n ? vals[lo] : 0.f; vhi = n ? vals[hi - 1] : 0.f;
    __syncthreads();                                                 // vals is filled again by the caller
}
