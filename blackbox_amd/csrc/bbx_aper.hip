// bbx_aper.hip -- aperture photometry of the catalogue with a local sky annulus (include/bbx.h, bbx_aper_phot):
// per source the fluxes inside circles of radii[k] x FWHM with the exact circle-pixel overlap as weight, and the clipped median
// of the pixels whose centres lie in the annulus [sky_in, sky_out) x FWHM.
//
//   k_aper_phot : one workgroup of 256 per source, all geometry in float64 (the Makefile's -ffp-contract=off keeps d^2 unfused)
//     1 sky     the annulus' used pixels -> LDS (appended per wave: one LDS atomic a wave and round; the order of arrival does
//               not reach the result, the sample is sorted next), then stats_clip<256> of bbx_stats.h: the one sort and clip
//               that bbx_match.hip and bbx_shapes.hip run with 1024 threads
//     2 classes the window of the largest aperture once more: a pixel inside aperture k adds itself with weight 1; one the
//               circle crosses is noted in the wave's own list of that aperture (in the sample's LDS, which is free by now)
//     3 arcs    the lists, 64 entries at a time: only here sqrt and asin in float64 are paid, by full waves
//     4 sums    S, A, V of every aperture: per thread in pixel order, then its list entries, the wave by DPP, the four waves in
//               order: no float atomics, the same input gives the same bits
#include "bbx_spline.h"
#include "bbx_stats.h"

#define APR_BLOCK  256
#define APR_WAVES  (APR_BLOCK / 64)
#define APR_NMAX   BBX_APER_NMAX
// the annulus sample: pixel centres inside a circle of at most BBX_APER_RMAX = 48 px, of which there are at most
// pi (48 + 0.71)^2 = 7454 -- BBX_MATCH_CAP = 8192 floats (32 KB) cannot overflow (the append is guarded all the same)
#define APR_CAP    BBX_MATCH_CAP
// the crossed pixels of one aperture noted by one wave: a circle of 48 px crosses about 8 r = 384 pixels, shared by four waves.
// 4 waves x 8 apertures x 512 window indices (uint16) = the sample's 32 KB.  A wave whose list is full takes the arc on the spot
#define APR_LCAP   512
#define APR_OFFMAX 1.0e6f
static_assert(APR_WAVES * APR_NMAX * APR_LCAP * 2 <= APR_CAP * 4, "the lists live in the sample buffer");
static_assert((2 * BBX_APER_RMAX + 2) * (2 * BBX_APER_RMAX + 2) < 65536, "a window index fits a list entry");

struct apr_args {
    const float* D; const float* sigma; const uint8_t* mask;
    const int32_t* ys; const int32_t* xs; const float* off; const float* fwhm;
    float* flux; float* err; float* sky; uint8_t* flags;
    int ny, nx, size, nsy, nsx, naper, sub_sky, sky_nmin;
    float radii[APR_NMAX];
    float sky_in, sky_out;
};

// ---- the overlap of a disc and a unit pixel -----------------------------------------------------------------------------
// antiderivative of sqrt(r^2 - x^2)
__device__ __forceinline__ double apr_G(double x, double r, double r2) {
    const double q = fmax(r2 - x * x, 0.0);
    const double t = fmin(fmax(x / r, -1.0), 1.0);
    return 0.5 * (x * sqrt(q) + r2 * asin(t));
}
__device__ __forceinline__ void apr_order(double& a, double& b) { const double lo = fmin(a, b), hi = fmax(a, b); a = lo; b = hi; }

// area of the disc of radius r about the origin inside the unit pixel centred on (ax, ay): the clipped chord height integrated
// over the pixel's x-range, split at +-sqrt(r^2 - y0^2), +-sqrt(r^2 - y1^2) (y0, y1: the pixel's lower and upper edge); the form
// of each piece (flat edge or arc, top and bottom) is decided at its midpoint
__device__ __noinline__ double apr_partial(double ax, double ay, double r, double r2) {
    const double x0 = ax - 0.5, x1 = ax + 0.5, y0 = ay - 0.5, y1 = ay + 0.5;
    const double a = fmax(x0, -r), b = fmin(x1, r);
    const double c0 = sqrt(fmax(r2 - y0 * y0, 0.0)), c1 = sqrt(fmax(r2 - y1 * y1, 0.0));
    double p[6];
    p[0] = a; p[5] = b;
    p[1] = fmin(fmax(-c0, a), b); p[2] = fmin(fmax(c0, a), b); p[3] = fmin(fmax(-c1, a), b); p[4] = fmin(fmax(c1, a), b);
    apr_order(p[1], p[2]); apr_order(p[3], p[4]); apr_order(p[1], p[3]); apr_order(p[2], p[4]); apr_order(p[2], p[3]);
    double g[6];
#pragma unroll
    for (int i = 0; i < 6; i++) g[i] = apr_G(p[i], r, r2);
    double area = 0.0;
#pragma unroll
    for (int i = 0; i < 5; i++) {
        const double lo = p[i], hi = p[i + 1];
        const double m = 0.5 * (lo + hi);
        const double h = sqrt(fmax(r2 - m * m, 0.0));
        const double arc = g[i + 1] - g[i];
        const double top = y1 <= h ? y1 * (hi - lo) : arc;
        const double bot = y0 >= -h ? y0 * (hi - lo) : -arc;
        const bool on = hi > lo && fmin(y1, h) > fmax(y0, -h);
        area = area + (on ? top - bot : 0.0);
    }
    return fmin(fmax(area, 0.0), 1.0);                               // (rounding may leave the sum a few 1e-17 outside)
}

// ---- the kernel -------------------------------------------------------------------------------------------------------------
// pixel (y, x) of the frame (on it): is it used, and its D and sigma
template <bool MINI>
__device__ __forceinline__ bool apr_pixel(const apr_args& a, const bbx_spl& sp, long long y, long long x, float& d, float& sg) {
    const size_t ix = (size_t)y * (size_t)a.nx + (size_t)x;
    if (a.mask && a.mask[ix]) return false;
    d = a.D[ix];
    if (!finite_f32(d)) return false;
    sg = MINI ? bbx_spl_eval(sp, (int)y, (int)x) : a.sigma[ix];
    return finite_f32(sg);
}

// the window of the pixels a circle of radius R about the offset o may touch, relative to the integer peak: [lo, lo + w)
__device__ __forceinline__ void apr_window(double o, double R, int& lo, int& w) {
    lo = (int)ceil(o - R - 0.5);
    w = (int)floor(o + R + 0.5) - lo + 1;
    if (w < 0) w = 0;
}

template <bool MINI>
__global__ __launch_bounds__(APR_BLOCK) void k_aper_phot(apr_args a, bbx_spl sp) {
    __shared__ __attribute__((aligned(16))) float s_vals[APR_CAP];   // 32 KB: the annulus sample, then the lists of crossed pixels
    __shared__ double s_red[2 * 2 * APR_WAVES];
    __shared__ double s_sum[APR_WAVES][3 * APR_NMAX];
    __shared__ int s_cnt;
    __shared__ unsigned s_fl;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t s = blockIdx.x;
    const long long yp = a.ys[s], xp = a.xs[s];
    const double nan = __builtin_nan("");
    // ---- centre, FWHM, radii (all uniform per workgroup)
    double oy = 0.0, ox = 0.0;
    unsigned fl = 0;
    if (a.off) {
        const float fy = a.off[2 * s], fx = a.off[2 * s + 1];
        if (finite_f32(fy) && finite_f32(fx) && fabsf(fy) <= APR_OFFMAX && fabsf(fx) <= APR_OFFMAX) { oy = (double)fy; ox = (double)fx; }
        else fl |= 1u;
    }
    const int ty = (int)min(max(yp / a.size, 0ll), (long long)a.nsy - 1), tx = (int)min(max(xp / a.size, 0ll), (long long)a.nsx - 1);
    const float f = a.fwhm[ty * a.nsx + tx];
    double rk[APR_NMAX], r2k[APR_NMAX], rmax = 0.0;
#pragma unroll
    for (int k = 0; k < APR_NMAX; k++) {
        rk[k] = k < a.naper ? (double)a.radii[k] * (double)f : 0.0;
        r2k[k] = rk[k] * rk[k];
        rmax = fmax(rmax, rk[k]);
    }
    const double r_in = (double)a.sky_in * (double)f, r_out = (double)a.sky_out * (double)f;
    if (!(finite_f32(f) && f > 0.f) || rmax > (double)BBX_APER_RMAX || r_out > (double)BBX_APER_RMAX) {      // too big: nothing is measured
        if (tid < a.naper) { a.flux[s * a.naper + tid] = (float)nan; a.err[s * a.naper + tid] = (float)nan; }
        if (tid == 0) { a.sky[3 * s] = (float)nan; a.sky[3 * s + 1] = (float)nan; a.sky[3 * s + 2] = 0.f; a.flags[s] = (uint8_t)(fl | 32u); }
        return;
    }
    if (tid == 0) { s_cnt = 0; s_fl = 0u; }
    __syncthreads();
    // ---- 1: the local sky
    {
        const double rin2 = r_in * r_in, rout2 = r_out * r_out;
        int ylo, xlo, wy, wx;
        apr_window(oy, r_out, ylo, wy);
        apr_window(ox, r_out, xlo, wx);
        const int npx = wy * wx;
        for (int b = wave * 64; b < npx; b += APR_BLOCK) {           // (the same trips for every lane of a wave)
            const int j = b + lane;
            bool take = false;
            float d = 0.f, sg;
            if (j < npx) {
                const int jy = j / wx, jx = j - jy * wx;
                const double dy = (double)(ylo + jy) - oy, dx = (double)(xlo + jx) - ox;
                const double d2 = dy * dy + dx * dx;
                if (d2 >= rin2 && d2 < rout2) {
                    const long long y = yp + ylo + jy, x = xp + xlo + jx;
                    take = y >= 0 && y < a.ny && x >= 0 && x < a.nx && apr_pixel<MINI>(a, sp, y, x, d, sg);
                    if (!take) fl |= 16u;
                }
            }
            const unsigned long long m = __ballot(take);
            if (m) {                                                 // (uniform)
                int base = 0;
                if (lane == 0) base = atomicAdd(&s_cnt, (int)__popcll(m));
                base = __builtin_amdgcn_readfirstlane(base);
                const int pos = base + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                if (take && pos < APR_CAP) s_vals[pos] = d;
            }
        }
    }
    __syncthreads();
    const int msky = min(s_cnt, APR_CAP);
    double st[4];                                                    // n, median, mean (not used), std
    float vlo, vhi;
    int ph = 0;
    stats_clip<APR_BLOCK>(s_vals, msky, s_red, ph, st, vlo, vhi);    // (ends behind a barrier: s_vals is free)
    const bool few = st[0] < (double)a.sky_nmin;
    if (few) fl |= 8u;
    const bool subtract = a.sub_sky && !few;
    // ---- 2: the apertures' pixels by class
    double S[APR_NMAX], A[APR_NMAX], V[APR_NMAX];
    int cnt[APR_NMAX];
#pragma unroll
    for (int k = 0; k < APR_NMAX; k++) { S[k] = A[k] = V[k] = 0.0; cnt[k] = 0; }
    uint16_t* lst = (uint16_t*)s_vals + (size_t)wave * APR_NMAX * APR_LCAP;
    int ylo, xlo, wy, wx;
    apr_window(oy, rmax, ylo, wy);
    apr_window(ox, rmax, xlo, wx);
    const int npx = wy * wx;
    const double r2max = rmax * rmax;
    for (int b = wave * 64; b < npx; b += APR_BLOCK) {
        const int j = b + lane;
        bool used = false;
        float d = 0.f, sg = 0.f;
        double ay = 0.0, ax = 0.0, far = 0.0, near = 0.0;
        if (j < npx) {
            const int jy = j / wx, jx = j - jy * wx;
            ay = fabs((double)(ylo + jy) - oy); ax = fabs((double)(xlo + jx) - ox);
            const double fy = ay + 0.5, fx = ax + 0.5, my = fmax(ay - 0.5, 0.0), mx = fmax(ax - 0.5, 0.0);
            far = fx * fx + fy * fy;
            near = mx * mx + my * my;
            if (near < r2max) {                                      // the largest aperture touches the pixel
                const long long y = yp + ylo + jy, x = xp + xlo + jx;
                if (!(y >= 0 && y < a.ny && x >= 0 && x < a.nx)) fl |= 4u;
                else if (!(used = apr_pixel<MINI>(a, sp, y, x, d, sg))) fl |= 2u;
            }
        }
        const double dd = (double)d, var = (double)(fmaxf(d, 0.f) + sg * sg);
#pragma unroll
        for (int k = 0; k < APR_NMAX; k++) {
            if (k >= a.naper) break;                                 // (uniform)
            const bool full = used && far <= r2k[k];
            const bool part = used && !full && near < r2k[k];
            if (full) { S[k] += dd; A[k] += 1.0; V[k] += var; }
            const unsigned long long m = __ballot(part);
            if (m) {
                const int pos = cnt[k] + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                if (part) {
                    if (pos < APR_LCAP) lst[k * APR_LCAP + pos] = (uint16_t)j;
                    else {                                           // the list is full: on the spot
                        const double w = apr_partial(ax, ay, rk[k], r2k[k]);
                        S[k] += w * dd; A[k] += w; V[k] += w * var;
                    }
                }
                cnt[k] += (int)__popcll(m);
            }
        }
    }
    __syncthreads();
    // ---- 3: the crossed pixels, every wave its own lists
#pragma unroll
    for (int k = 0; k < APR_NMAX; k++) {
        if (k >= a.naper) break;
        const int n = min(cnt[k], APR_LCAP);
        for (int e = lane; e < n; e += 64) {
            const int j = lst[k * APR_LCAP + e];
            const int jy = j / wx, jx = j - jy * wx;
            const double ay = fabs((double)(ylo + jy) - oy), ax = fabs((double)(xlo + jx) - ox);
            float d = 0.f, sg = 0.f;
            apr_pixel<MINI>(a, sp, yp + ylo + jy, xp + xlo + jx, d, sg);          // (a used pixel of the frame: noted as such)
            const double w = apr_partial(ax, ay, rk[k], r2k[k]);
            const double var = (double)(fmaxf(d, 0.f) + sg * sg);
            S[k] += w * (double)d; A[k] += w; V[k] += w * var;
        }
    }
    // ---- 4: the sums and the outputs
#pragma unroll
    for (int k = 0; k < APR_NMAX; k++) {
        if (k >= a.naper) break;
        const double ws = wave_sum_f64(S[k]), wa = wave_sum_f64(A[k]), wv = wave_sum_f64(V[k]);
        if (lane == 0) { s_sum[wave][3 * k] = ws; s_sum[wave][3 * k + 1] = wa; s_sum[wave][3 * k + 2] = wv; }
    }
    if (fl) atomicOr(&s_fl, fl);
    __syncthreads();
    if (tid < a.naper) {
        const int k = tid;
        double t[3];
#pragma unroll
        for (int q = 0; q < 3; q++) t[q] = ((s_sum[0][3 * k + q] + s_sum[1][3 * k + q]) + s_sum[2][3 * k + q]) + s_sum[3][3 * k + q];
        const double Sk = t[0], Ak = t[1], Vk = t[2];
        double F = Sk, E2 = Vk;
        if (subtract) {
            F = Sk - st[1] * Ak;
            E2 = Vk + Ak * Ak * (3.141592653589793 / 2.0) * st[3] * st[3] / st[0];
        }
        const bool none = Ak == 0.0;
        a.flux[s * a.naper + k] = none ? (float)nan : (float)F;
        a.err[s * a.naper + k] = none ? (float)nan : (float)sqrt(E2);
    }
    if (tid == 0) {
        a.sky[3 * s] = few ? (float)nan : (float)st[1];
        a.sky[3 * s + 1] = few ? (float)nan : (float)st[3];
        a.sky[3 * s + 2] = (float)st[0];
        a.flags[s] = (uint8_t)s_fl;
    }
}

extern "C" int bbx_aper_phot(bbx_ctx* ctx, int ny, int nx, const float* d_D, const float* d_sigma, const bbx_spline_image* sigma_mini,
                             const uint8_t* d_mask, int nsrc, const int32_t* d_ys, const int32_t* d_xs, const float* d_off,
                             const float* d_fwhm, int size, int nsy, int nsx, int naper, const float* radii, float sky_in, float sky_out,
                             int sub_sky, int sky_nmin, float* d_flux, float* d_err, float* d_sky, uint8_t* d_flags, void* stream) {
    if (!ctx || ny < 1 || nx < 1 || nsrc < 0 || size < 1 || nsy < 1 || nsx < 1 || naper < 1 || naper > APR_NMAX || !radii || sky_nmin < 1)
        return BBX_ERR_ARG;
    if (!(sky_in >= 0.f) || !(sky_out > sky_in) || !(sky_out < 3.0e38f)) return BBX_ERR_ARG;
    if ((d_sigma != nullptr) == (sigma_mini != nullptr)) return BBX_ERR_ARG;                // one form
    apr_args a = {};
    for (int k = 0; k < naper; k++) {
        if (!(radii[k] > 0.f) || !(radii[k] < 3.0e38f)) return BBX_ERR_ARG;
        a.radii[k] = radii[k];
    }
    bbx_spl sp = {};
    if (sigma_mini) {
        const int rc = bbx_spl_make(sigma_mini, ny, nx, &sp);
        if (rc) return rc;
    }
    if (nsrc == 0) return BBX_OK;
    if (!d_D || !d_ys || !d_xs || !d_fwhm || !d_flux || !d_err || !d_sky || !d_flags) return BBX_ERR_ARG;
    a.D = d_D; a.sigma = d_sigma; a.mask = d_mask; a.ys = d_ys; a.xs = d_xs; a.off = d_off; a.fwhm = d_fwhm;
    a.flux = d_flux; a.err = d_err; a.sky = d_sky; a.flags = d_flags;
    a.ny = ny; a.nx = nx; a.size = size; a.nsy = nsy; a.nsx = nsx; a.naper = naper; a.sub_sky = sub_sky ? 1 : 0; a.sky_nmin = sky_nmin;
    a.sky_in = sky_in; a.sky_out = sky_out;
    if (sigma_mini)
        hipLaunchKernelGGL(k_aper_phot<true>, dim3(nsrc), dim3(APR_BLOCK), 0, (hipStream_t)stream, a, sp);
    else
        hipLaunchKernelGGL(k_aper_phot<false>, dim3(nsrc), dim3(APR_BLOCK), 0, (hipStream_t)stream, a, sp);
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}
