// bbx_shapes.hip -- source shapes of the full-source catalogue: FWHM, ELONGATION, THETA per source from adaptive second
// moments (Bernstein & Jarvis 2002, AJ 123, 583; Hirata & Seljak 2003, MNRAS 343, 459), and the per-tile / per-frame
// clipped statistics behind the header keys S-FWHM, S-FWSTD, S-SEEING, S-SEESTD, S-ELONG, S-ELOSTD (blackbox.py:3051-3057).
//
//   k_src_shapes  : one wave per source, as k_win_centroid: the window pixels stay in registers over the iterations, no LDS
//   k_shape_stats : one workgroup per sub-image tile + one for the frame, the selection, sort and clipping of bbx_stats.h
#include "bbx_stats.h"

#define SHP_BLOCK   256
#define SHP_RMAX    10
#define SHP_NREG    7                                    // ceil((2 * 10 + 1)^2 / 64)

// ---------------------------------------------------------------------------------------------------------------------
// adaptive second moments
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SHP_BLOCK) void k_src_shapes(int ny, int nx, const float* __restrict__ img, const uint8_t* __restrict__ mask,
                                                          int nsrc, const int32_t* __restrict__ ys, const int32_t* __restrict__ xs,
                                                          const float* __restrict__ off, const float* __restrict__ sigw, int size, int nsy,
                                                          int nsx, int R, int niter, float* __restrict__ out, uint8_t* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int src = blockIdx.x * (SHP_BLOCK / 64) + (threadIdx.x >> 6);
    if (src >= nsrc) return;                                         // (uniform per wave)
    const int yc = ys[src], xc = xs[src];
    const int W = 2 * R + 1, npx = W * W;
    float I[SHP_NREG], py[SHP_NREG], px[SHP_NREG];
    unsigned fl = 0;
#pragma unroll
    for (int j = 0; j < SHP_NREG; j++) {
        const int k = lane + 64 * j;
        const int r = k / W, c = k - r * W;
        const long long y = (long long)yc + r - R, x = (long long)xc + c - R;
        float v = 0.f;                                               // off the frame (and past the window): contributes nothing
        if (k < npx && y >= 0 && y < ny && x >= 0 && x < nx) {
            v = img[(size_t)y * nx + x];
            if (mask) fl |= mask[(size_t)y * nx + x];
        }
        I[j] = v; py[j] = (float)(r - R); px[j] = (float)(c - R);
    }
    unsigned wfl = 0;                                                // OR over the wave, bit by bit
#pragma unroll
    for (int b = 0; b < 8; b++)
        if (__ballot((fl >> b) & 1u)) wfl |= 1u << b;

    const int ty = min(max(yc / size, 0), nsy - 1), tx = min(max(xc / size, 0), nsx - 1);
    const float sg = sigw[ty * nsx + tx];
    const float lim = 0.5f * (float)R, tmax = 2.0f * (lim * lim);
    float cy = off[2 * (size_t)src], cx = off[2 * (size_t)src + 1];
    float ayy = 1.0f / (sg * sg), axx = ayy, axy = 0.f;              // W^-1
    float Tyy = 0.f, Txx = 0.f, Txy = 0.f;
    bool ok = finite_f32(cy) && finite_f32(cx) && sg > 0.f && finite_f32(sg) && finite_f32(ayy);
    for (int it = 0; it < niter && ok; it++) {                       // (ok is the same in every lane: it follows from wave sums)
        float s0 = 0.f, sy = 0.f, sx = 0.f, syy = 0.f, sxx = 0.f, sxy = 0.f;
#pragma unroll
        for (int j = 0; j < SHP_NREG; j++) {
            const float dy = py[j] - cy, dx = px[j] - cx;
            const float q = (ayy * (dy * dy) + axx * (dx * dx)) + (2.0f * axy) * (dy * dx);
            const float w = expf(-0.5f * q) * I[j];
            const float wy = w * dy, wx = w * dx;
            s0 += w; sy += wy; sx += wx; syy += wy * dy; sxx += wx * dx; sxy += wy * dx;
        }
        s0 = wave_sum_f32(s0); sy = wave_sum_f32(sy); sx = wave_sum_f32(sx);
        syy = wave_sum_f32(syy); sxx = wave_sum_f32(sxx); sxy = wave_sum_f32(sxy);
        ok = s0 > 0.f && finite_f32(s0) && finite_f32(sy) && finite_f32(sx) && finite_f32(syy) && finite_f32(sxx) &&
             finite_f32(sxy);
        if (!ok) break;
        const float my = sy / s0, mx = sx / s0;
        const float Myy = syy / s0 - my * my, Mxx = sxx / s0 - mx * mx, Mxy = sxy / s0 - my * mx;
        const float dM = Myy * Mxx - Mxy * Mxy;
        cy = cy + 2.0f * my; cx = cx + 2.0f * mx;
        ok = dM > 0.f && Myy > 0.f && finite_f32(dM) && finite_f32(cy) && finite_f32(cx) && fabsf(cy) <= lim && fabsf(cx) <= lim;
        if (!ok) break;
        const float byy = Mxx / dM - ayy, bxx = Myy / dM - axx, bxy = -Mxy / dM - axy;        // T^-1 = M^-1 - W^-1
        const float dT = byy * bxx - bxy * bxy;
        ok = dT > 0.f && byy > 0.f && finite_f32(dT);
        if (!ok) break;
        Tyy = bxx / dT; Txx = byy / dT; Txy = -bxy / dT;
        ok = finite_f32(Tyy) && finite_f32(Txx) && finite_f32(Txy) && Tyy + Txx <= tmax;
        ayy = byy; axx = bxx; axy = bxy;                             // W <- T
    }
    const float tr = Tyy + Txx, df = Txx - Tyy;
    const float rad = sqrtf(df * df + 4.0f * (Txy * Txy));
    const float A2 = (tr + rad) / 2.0f, B2 = (tr - rad) / 2.0f;
    const float fwhm = 2.0f * sqrtf(0.6931471805599453f * tr);
    const float elong = sqrtf(A2 / B2);
    const float theta = (0.5f * atan2f(2.0f * Txy, df)) * 57.29577951308232f;
    ok = ok && finite_f32(fwhm) && finite_f32(elong) && finite_f32(theta);
    if (lane == 0) {
        flags[src] = (uint8_t)wfl;                                   // (for failed sources too)
        const float nan = __builtin_nanf("");
        float* o = out + 8 * (size_t)src;
        o[0] = ok ? cy : nan; o[1] = ok ? cx : nan; o[2] = ok ? Tyy : nan; o[3] = ok ? Txx : nan; o[4] = ok ? Txy : nan;
        o[5] = ok ? fwhm : nan; o[6] = ok ? elong : nan; o[7] = ok ? theta : nan;
    }
}

extern "C" int bbx_src_shapes(bbx_ctx* ctx, int ny, int nx, const float* d_img, const uint8_t* d_mask, int nsrc, const int32_t* d_ys,
                              const int32_t* d_xs, const float* d_off, const float* d_sigw, int size, int nsy, int nsx, int radius,
                              int niter, float* d_out, uint8_t* d_flags, void* stream) {
    if (!ctx || ny < 1 || nx < 1 || nsrc < 0 || size < 1 || nsy < 1 || nsx < 1 || radius < 1 || radius > SHP_RMAX || niter < 1)
        return BBX_ERR_ARG;
    if (nsrc == 0) return BBX_OK;
    if (!d_img || !d_ys || !d_xs || !d_off || !d_sigw || !d_out || !d_flags) return BBX_ERR_ARG;
    const int per = SHP_BLOCK / 64;
    hipLaunchKernelGGL(k_src_shapes, dim3((nsrc + per - 1) / per), dim3(SHP_BLOCK), 0, (hipStream_t)stream, ny, nx, d_img, d_mask, nsrc,
                       d_ys, d_xs, d_off, d_sigw, size, nsy, nsx, radius, niter, d_out, d_flags);
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// clipped statistics of FWHM and ELONGATION per sub-image tile and of the frame
// ---------------------------------------------------------------------------------------------------------------------
struct shape_in {
    const int32_t* ys; const int32_t* xs; const float* shapes; const uint8_t* flags; const float* flux; const float* err;
    int n;
    float snr_min;
};
enum { SQ_COUNT = 0, SQ_FWHM, SQ_ELONG };

template <int Q>
struct shape_item {
    const shape_in& in;
    float* __restrict__ vals;
    float fw, el;
    __device__ __forceinline__ bool load(int i, const stats_seg& sg) {
        const int y = in.ys[i], x = in.xs[i];
        const float f = in.flux[i], e = in.err[i];
        fw = in.shapes[8 * (size_t)i + 5]; el = in.shapes[8 * (size_t)i + 6];
        return finite_f32(fw) && finite_f32(el) && in.flags[i] == 0 && e > 0.f && f / e >= in.snr_min &&
               y >= sg.y0 && y < sg.y1 && x >= sg.x0 && x < sg.x1;
    }
    __device__ __forceinline__ void put(int, int pos) { vals[pos] = Q == SQ_FWHM ? fw : el; }
};

__global__ __launch_bounds__(STATS_BLOCK) void k_shape_stats(shape_in in, int size, int nsy, int nsx, double* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float s_vals[BBX_MATCH_CAP];                         // 32 KB: one quantity at a time
    __shared__ double s_red[2 * 2 * STATS_WAVES];
    __shared__ int s_cnt[STATS_WAVES];
    const int tid = threadIdx.x;
    const int seg = blockIdx.x;
    stats_seg sg = stats_segment(seg, size, nsy, nsx, in.ys, in.n);
    int base;
    shape_item<SQ_COUNT> cnt = {in, s_vals};
    const int n = stats_count(sg, cnt, s_cnt, base);
    const int m = (n + sg.stride - 1) / sg.stride;                   // <= BBX_MATCH_CAP
    double* o = out + (size_t)seg * 8;
    if (n == 0) {                                                    // (uniform per workgroup)
        if (tid == 0) {
            const double nan = __builtin_nan("");
            o[0] = 0.0; o[1] = 1.0; o[2] = 0.0; o[3] = nan; o[4] = nan; o[5] = 0.0; o[6] = nan; o[7] = nan;
        }
        return;
    }
    int ph = 0;
    double st[4];
    float vlo, vhi;
    shape_item<SQ_FWHM> fw = {in, s_vals};
    stats_walk<false>(sg, base, fw);
    __syncthreads();
    stats_clip<STATS_BLOCK>(s_vals, m, s_red, ph, st, vlo, vhi);
    if (tid == 0) { o[0] = (double)n; o[1] = (double)sg.stride; o[2] = st[0]; o[3] = st[1]; o[4] = st[3]; }
    shape_item<SQ_ELONG> el = {in, s_vals};
    stats_walk<false>(sg, base, el);
    __syncthreads();
    stats_clip<STATS_BLOCK>(s_vals, m, s_red, ph, st, vlo, vhi);
    if (tid == 0) { o[5] = st[0]; o[6] = st[1]; o[7] = st[3]; }
}

extern "C" int bbx_shape_stats(bbx_ctx* ctx, int nsrc, const int32_t* d_ys, const int32_t* d_xs, const float* d_shapes,
                               const uint8_t* d_flags, const float* d_flux, const float* d_err, int size, int nsy, int nsx, float snr_min,
                               double* d_out, void* stream) {
    if (!ctx || nsrc < 0 || size < 1 || nsy < 1 || nsx < 1 || (long long)nsy * nsx > 65535) return BBX_ERR_ARG;
    if (nsrc == 0) return BBX_OK;
    if (!d_ys || !d_xs || !d_shapes || !d_flags || !d_flux || !d_err || !d_out) return BBX_ERR_ARG;
    const shape_in in = {d_ys, d_xs, d_shapes, d_flags, d_flux, d_err, nsrc, snr_min};
    hipLaunchKernelGGL(k_shape_stats, dim3(nsy * nsx + 1), dim3(STATS_BLOCK), 0, (hipStream_t)stream, in, size, nsy, nsx, d_out);
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}
