// bbx_match.hip -- flux ratio and astrometric scatter from matched stars (buildref.py:2782-3014 get_fratio, "simplified
// version of zogy.get_fratio_dxdy"; [EXT] get_fratio_dxdy, get_matches, get_mean_fratio are not in the reference tree).
//
//   k_win_centroid : one wave per source; the window pixels stay in registers over the iterations, no LDS
//   k_match_nearest: one thread per source; binary search of the other list's row band, scan of the band (two launches)
//   k_match_stats  : one workgroup per sub-image tile + one for the frame; count, strided selection in list order, LDS sort,
//                    sigma clipping on the sorted sample (oracle/zogy_core.box_stats), float64 sums in a fixed order
#include "bbx_stats.h"

#define MATCH_BLOCK   256
#define CEN_RMAX      10
#define CEN_NREG      7                                  // ceil((2 * 10 + 1)^2 / 64)

// ---------------------------------------------------------------------------------------------------------------------
// windowed centroid (the wave sum: bbx_common.h)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MATCH_BLOCK) void k_win_centroid(int ny, int nx, const float* __restrict__ img, int nsrc,
                                                              const int32_t* __restrict__ ys, const int32_t* __restrict__ xs,
                                                              const float* __restrict__ sigw, int size, int nsy, int nsx, int R, int niter,
                                                              float* __restrict__ off) {
    const int lane = threadIdx.x & 63;
    const int src = blockIdx.x * (MATCH_BLOCK / 64) + (threadIdx.x >> 6);
    if (src >= nsrc) return;                                         // (uniform per wave)
    const int yc = ys[src], xc = xs[src];
    const int W = 2 * R + 1, npx = W * W;
    float I[CEN_NREG], py[CEN_NREG], px[CEN_NREG];
#pragma unroll
    for (int j = 0; j < CEN_NREG; j++) {
        const int k = lane + 64 * j;
        const int r = k / W, c = k - r * W;
        const long long y = (long long)yc + r - R, x = (long long)xc + c - R;
        float v = 0.f;                                               // off the frame (and past the window): contributes nothing
        if (k < npx && y >= 0 && y < ny && x >= 0 && x < nx) v = img[(size_t)y * nx + x];
        I[j] = v; py[j] = (float)(r - R); px[j] = (float)(c - R);
    }
    const int ty = min(max(yc / size, 0), nsy - 1), tx = min(max(xc / size, 0), nsx - 1);
    const float sg = sigw[ty * nsx + tx];
    const float inv = 1.0f / (2.0f * sg * sg);
    const float lim = 0.5f * (float)R;
    float cy = 0.f, cx = 0.f;
    bool ok = sg > 0.f && finite_f32(sg) && finite_f32(inv);
    for (int it = 0; it < niter && ok; it++) {                       // (ok is the same in every lane: it follows from wave sums)
        float sw = 0.f, sy = 0.f, sx = 0.f;
#pragma unroll
        for (int j = 0; j < CEN_NREG; j++) {
            const float dy = py[j] - cy, dx = px[j] - cx;
            const float w = expf(-(dy * dy + dx * dx) * inv) * I[j];
            sw += w; sy += w * dy; sx += w * dx;
        }
        sw = wave_sum_f32(sw); sy = wave_sum_f32(sy); sx = wave_sum_f32(sx);
        ok = sw > 0.f && finite_f32(sw) && finite_f32(sy) && finite_f32(sx);
        if (ok) {
            cy = cy + 2.0f * (sy / sw);
            cx = cx + 2.0f * (sx / sw);
            ok = finite_f32(cy) && finite_f32(cx) && fabsf(cy) <= lim && fabsf(cx) <= lim;
        }
    }
    if (lane == 0) {
        const float nan = __builtin_nanf("");
        off[2 * (size_t)src] = ok ? cy : nan;
        off[2 * (size_t)src + 1] = ok ? cx : nan;
    }
}

extern "C" int bbx_win_centroid(bbx_ctx* ctx, int ny, int nx, const float* d_img, int nsrc, const int32_t* d_ys, const int32_t* d_xs,
                                const float* d_sigw, int size, int nsy, int nsx, int radius, int niter, float* d_off, void* stream) {
    if (!ctx || ny < 1 || nx < 1 || nsrc < 0 || size < 1 || nsy < 1 || nsx < 1 || radius < 1 || radius > CEN_RMAX || niter < 0)
        return BBX_ERR_ARG;
    if (nsrc == 0) return BBX_OK;
    if (!d_img || !d_ys || !d_xs || !d_sigw || !d_off) return BBX_ERR_ARG;
    const int per = MATCH_BLOCK / 64;
    hipLaunchKernelGGL(k_win_centroid, dim3((nsrc + per - 1) / per), dim3(MATCH_BLOCK), 0, (hipStream_t)stream, ny, nx, d_img, nsrc,
                       d_ys, d_xs, d_sigw, size, nsy, nsx, radius, niter, d_off);
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// mutual nearest neighbours
// ---------------------------------------------------------------------------------------------------------------------
struct match_list { const int32_t* ys; const int32_t* xs; const float* off; int n; };

// nearest source of [o] to source i of [s] within dmax2 (float32 distance^2, inclusive), the lower index on ties; -1: none.
// The distance of a pair is the same float whichever side forms it: every term only changes sign.
__device__ __forceinline__ int match_nearest(const match_list& s, int i, const match_list& o, int band, float dmax2) {
    const float oy = s.off[2 * (size_t)i], ox = s.off[2 * (size_t)i + 1];
    if (!(oy == oy) || !(ox == ox)) return -1;
    const int y = s.ys[i], x = s.xs[i];
    int best = -1;
    float bd = 0.f;
    for (int j = match_lower_bound(o.ys, o.n, y - band); j < o.n; j++) {
        const int yj = o.ys[j];
        if (yj > y + band) break;
        const int xj = o.xs[j];
        if (xj < x - band || xj > x + band) continue;
        const float dy = (float)(yj - y) + (o.off[2 * (size_t)j] - oy);
        const float dx = (float)(xj - x) + (o.off[2 * (size_t)j + 1] - ox);
        const float d2 = dy * dy + dx * dx;
        if (d2 <= dmax2 && (best < 0 || d2 < bd)) { best = j; bd = d2; }         // (a NaN offset of j: d2 <= dmax2 is false)
    }
    return best;
}

// phase 0: best_b[b] = nearest a of every b.  phase 1: match[a] = nearest b of a where best_b[b] == a, else -1
__global__ __launch_bounds__(MATCH_BLOCK) void k_match_nearest(match_list A, match_list B, int band, float dmax2, int phase,
                                                               int32_t* __restrict__ best_b, int32_t* __restrict__ match) {
    const int i = blockIdx.x * MATCH_BLOCK + threadIdx.x;
    if (phase == 0) {
        if (i < B.n) best_b[i] = match_nearest(B, i, A, band, dmax2);
    } else if (i < A.n) {
        const int b = B.n ? match_nearest(A, i, B, band, dmax2) : -1;
        match[i] = (b >= 0 && best_b[b] == i) ? b : -1;
    }
}

extern "C" int bbx_match_mutual(bbx_ctx* ctx, int n_a, const int32_t* d_a_ys, const int32_t* d_a_xs, const float* d_a_off, int n_b,
                                const int32_t* d_b_ys, const int32_t* d_b_xs, const float* d_b_off, float dist_max, int32_t* d_best_b,
                                int32_t* d_match, void* stream) {
    if (!ctx || n_a < 0 || n_b < 0 || !(dist_max >= 0.f) || dist_max > 1024.f) return BBX_ERR_ARG;
    if (n_a == 0) return BBX_OK;
    if (!d_a_ys || !d_a_xs || !d_a_off || !d_match) return BBX_ERR_ARG;
    if (n_b > 0 && (!d_b_ys || !d_b_xs || !d_b_off || !d_best_b)) return BBX_ERR_ARG;
    const match_list A = {d_a_ys, d_a_xs, d_a_off, n_a}, B = {d_b_ys, d_b_xs, d_b_off, n_b};
    const int band = (int)ceilf(dist_max + 1.0f);
    const float dmax2 = dist_max * dist_max;
    if (n_b > 0) {
        hipLaunchKernelGGL(k_match_nearest, dim3((n_b + MATCH_BLOCK - 1) / MATCH_BLOCK), dim3(MATCH_BLOCK), 0, (hipStream_t)stream, A, B,
                           band, dmax2, 0, d_best_b, d_match);
        BBX_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_match_nearest, dim3((n_a + MATCH_BLOCK - 1) / MATCH_BLOCK), dim3(MATCH_BLOCK), 0, (hipStream_t)stream, A, B, band,
                       dmax2, 1, d_best_b, d_match);
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// clipped statistics per sub-image tile and of the frame
// ---------------------------------------------------------------------------------------------------------------------
struct stats_in {
    const int32_t* a_ys; const int32_t* a_xs; const float* a_off; const float* a_flux; const float* a_err;
    const int32_t* b_ys; const int32_t* b_xs; const float* b_off; const float* b_flux; const float* b_err;
    const int32_t* match;
    int n_a, n_b;
    float snr_min;
};
enum { Q_COUNT = 0, Q_FR, Q_DX, Q_DY, Q_WEIGHT };

// what stats_walk (bbx_stats.h) asks of list A.  Q_COUNT: only the qualification.  Q_FR / Q_DX / Q_DY: the selected pair puts
// its value into vals[pos].  Q_WEIGHT: the selected pairs with wlo <= fr <= whi add 1 / sigma^2 and fr / sigma^2 to
// (acc0, acc1), float64
template <int Q>
struct match_item {
    const stats_in& in;
    float* __restrict__ vals;
    float wlo, whi;
    double acc0, acc1;
    float fa, fb, ea, eb;
    int m, ya, xa;
    __device__ __forceinline__ bool load(int i, const stats_seg& sg) {
        m = in.match[i];
        if (m < 0 || m >= in.n_b) return false;
        ya = in.a_ys[i]; xa = in.a_xs[i];
        fa = in.a_flux[i]; ea = in.a_err[i]; fb = in.b_flux[m]; eb = in.b_err[m];
        return fa > 0.f && fb > 0.f && fa / ea >= in.snr_min && fb / eb >= in.snr_min &&
               ya >= sg.y0 && ya < sg.y1 && xa >= sg.x0 && xa < sg.x1;
    }
    __device__ __forceinline__ void put(int i, int pos) {
        const float fr = fa / fb;
        if (Q == Q_FR) vals[pos] = fr;
        if (Q == Q_DX) vals[pos] = (float)(xa - in.b_xs[m]) + (in.a_off[2 * (size_t)i + 1] - in.b_off[2 * (size_t)m + 1]);
        if (Q == Q_DY) vals[pos] = (float)(ya - in.b_ys[m]) + (in.a_off[2 * (size_t)i] - in.b_off[2 * (size_t)m]);
        if (Q == Q_WEIGHT && fr >= wlo && fr <= whi) {
            // buildref.py:2969-2971: fratio * sqrt((e_new / f_new)^2 + (e_ref / f_ref)^2)
            const double ra = (double)ea / (double)fa, rb = (double)eb / (double)fb;
            const double s = (double)fr * sqrt(ra * ra + rb * rb);
            const double w = 1.0 / (s * s);
            acc0 += w; acc1 += w * (double)fr;
        }
    }
};
template <int Q>
__device__ __forceinline__ void match_walk(const stats_in& in, const stats_seg& sg, int base, float* __restrict__ vals, float wlo, float whi,
                                           double& acc0, double& acc1) {
    match_item<Q> it = {in, vals, wlo, whi, acc0, acc1};
    stats_walk<false>(sg, base, it);
    acc0 = it.acc0; acc1 = it.acc1;
}

__global__ __launch_bounds__(STATS_BLOCK) void k_match_stats(stats_in in, int size, int nsy, int nsx, double* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float s_vals[BBX_MATCH_CAP];                         // 32 KB: one quantity at a time
    __shared__ double s_red[2 * 2 * STATS_WAVES];
    __shared__ int s_cnt[STATS_WAVES];
    const int tid = threadIdx.x;
    const int seg = blockIdx.x;
    stats_seg sg = stats_segment(seg, size, nsy, nsx, in.a_ys, in.n_a);
    double z0 = 0.0, z1 = 0.0;
    int base;
    match_item<Q_COUNT> cnt = {in, s_vals, 0.f, 0.f, 0.0, 0.0};
    const int n = stats_count(sg, cnt, s_cnt, base);
    const int m = (n + sg.stride - 1) / sg.stride;                   // <= BBX_MATCH_CAP

    double* o = out + (size_t)seg * 16;
    const double nan = __builtin_nan("");
    if (n == 0) {                                                    // (uniform per workgroup)
        if (tid == 0) {
            for (int k = 0; k < 16; k++) o[k] = nan;
            o[0] = o[1] = o[7] = o[11] = 0.0; o[15] = 1.0;
        }
        return;
    }
    int ph = 0;
    double st[4];
    float vlo, vhi;
    // ---- flux ratio, and the weighted mean over its clipped sample
    match_walk<Q_FR>(in, sg, base, s_vals, 0.f, 0.f, z0, z1);
    __syncthreads();
    stats_clip<STATS_BLOCK>(s_vals, m, s_red, ph, st, vlo, vhi);
    double sw[2] = {0.0, 0.0};                                       // sum of w, sum of w f
    if (st[0] > 0.0) match_walk<Q_WEIGHT>(in, sg, base, s_vals, vlo, vhi, sw[0], sw[1]);
    wg_sum_tree<STATS_WAVES>(sw, s_red, ph);
    if (tid == 0) {
        o[0] = (double)n; o[1] = st[0]; o[2] = st[1]; o[3] = st[2]; o[4] = st[3];
        o[5] = st[0] > 0.0 ? sw[1] / sw[0] : nan;
        o[6] = st[0] > 0.0 ? 1.0 / sqrt(sw[0]) : nan;
        o[15] = (double)sg.stride;
    }
    // ---- dx, dy
    match_walk<Q_DX>(in, sg, base, s_vals, 0.f, 0.f, z0, z1);
    __syncthreads();
    stats_clip<STATS_BLOCK>(s_vals, m, s_red, ph, st, vlo, vhi);
    if (tid == 0) { o[7] = st[0]; o[8] = st[1]; o[9] = st[2]; o[10] = st[3]; }
    match_walk<Q_DY>(in, sg, base, s_vals, 0.f, 0.f, z0, z1);
    __syncthreads();
    stats_clip<STATS_BLOCK>(s_vals, m, s_red, ph, st, vlo, vhi);
    if (tid == 0) { o[11] = st[0]; o[12] = st[1]; o[13] = st[2]; o[14] = st[3]; }
}

extern "C" int bbx_match_stats(bbx_ctx* ctx, int n_a, const int32_t* d_a_ys, const int32_t* d_a_xs, const float* d_a_off,
                               const float* d_a_flux, const float* d_a_err, int n_b, const int32_t* d_b_ys, const int32_t* d_b_xs,
                               const float* d_b_off, const float* d_b_flux, const float* d_b_err, const int32_t* d_match, int size,
                               int nsy, int nsx, float snr_min, double* d_out, void* stream) {
    if (!ctx || n_a < 0 || n_b < 0 || size < 1 || nsy < 1 || nsx < 1 || (long long)nsy * nsx > 65535) return BBX_ERR_ARG;
    if (n_a == 0) return BBX_OK;
    if (!d_a_ys || !d_a_xs || !d_a_off || !d_a_flux || !d_a_err || !d_match || !d_out) return BBX_ERR_ARG;
    if (n_b > 0 && (!d_b_ys || !d_b_xs || !d_b_off || !d_b_flux || !d_b_err)) return BBX_ERR_ARG;
    const stats_in in = {d_a_ys, d_a_xs, d_a_off, d_a_flux, d_a_err, d_b_ys, d_b_xs, d_b_off, d_b_flux, d_b_err, d_match, n_a, n_b, snr_min};
    hipLaunchKernelGGL(k_match_stats, dim3(nsy * nsx + 1), dim3(STATS_BLOCK), 0, (hipStream_t)stream, in, size, nsy, nsx, d_out);
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}
