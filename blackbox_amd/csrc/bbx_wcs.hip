// bbx_wcs.hip -- the sphere of the astrometric solution (the rules are THIS PROJECT'S OWN, stated in include/bbx.h and
// in float64 numpy by tests/astrometry_ref.py: std_of_sky, sky_of_std, cat_list_ref, pix2sky_ref, pair_stats_ref).
//
//   bbx_wcs_cat_list   : one lane per catalogue row: gnomonic projection about the pointing, the virtual grid, the star-list form of
//                        bbx_align_*; the eligible rows counted per wave, one integer add each
//   bbx_wcs_pix2sky    : one lane per position: T, CD0, the inverse projection
//   bbx_wcs_pair_stats : one workgroup: per thread over items t, t + 256, ... in index order, the 256 partial sums added in thread
//                        order by thread 0; means first, then the deviations about them
//
// These are latency kernels: at 2e6 rows bbx_wcs_cat_list reads 20 bytes and writes 24 per row and spends some hundred float64
// operations on them, which a lane per row covers; nothing here is worth LDS.  No float atomics: same input, same bits.  Every index
// a kernel reads with is checked against the extent the entry was given for that array.
#include "bbx_common.h"

#define WCS_BLOCK 256
#define WCS_D2R   0.017453292519943295      // pi / 180
#define WCS_R2D   57.29577951308232         // 180 / pi

struct wcs_geom { double cd[4]; double ra0, dec0; int ny, nx; };          // CD0 row-major [deg / pix], the pointing [deg], the frame

__device__ __forceinline__ bool finite_f64(double v) { return fabs(v) < __builtin_huge_val(); }   // (false for NaN)

// rule 1: (ra, dec) [deg] -> (xi, eta) [deg] about (ra0, dec0); false: not in the field
__device__ __forceinline__ bool wcs_std_of_sky(double ra, double dec, double ra0, double dec0, double* xi, double* eta) {
    const double da = (ra - ra0) * WCS_D2R, d = dec * WCS_D2R, d0 = dec0 * WCS_D2R;
    const double sd = sin(d), cd = cos(d), sd0 = sin(d0), cd0 = cos(d0), sa = sin(da), ca = cos(da);
    const double D = sd0 * sd + cd0 * cd * ca;
    const double x = (cd * sa / D) * WCS_R2D, e = ((cd0 * sd - sd0 * cd * ca) / D) * WCS_R2D;
    *xi = x; *eta = e;
    return D > 0.0 && finite_f64(x) && finite_f64(e);
}

// rule 1, inverse: (xi, eta) [deg] -> (ra in [0, 360), dec) [deg]
__device__ __forceinline__ void wcs_sky_of_std(double xi, double eta, double ra0, double dec0, double* ra, double* dec) {
    const double x = xi * WCS_D2R, e = eta * WCS_D2R, d0 = dec0 * WCS_D2R;
    const double sd0 = sin(d0), cd0 = cos(d0);
    const double den = cd0 - e * sd0;
    double a = ra0 + atan2(x, den) * WCS_R2D;
    a = a - 360.0 * floor(a / 360.0);
    if (a >= 360.0) a = 0.0;
    *ra = a;
    *dec = atan2(sd0 + e * cd0, hypot(x, den)) * WCS_R2D;
}

// T at the frame position (x, y): bbx_align_grid's operations
__device__ __forceinline__ void wcs_T(const double* c, int ny, int nx, double x, double y, double* X, double* Y) {
    const double hy = 0.5 * (double)ny, hx = 0.5 * (double)nx;
    const double u = (x - hx) / hx, v = (y - hy) / hy;
    const double b[6] = {1.0, u, v, u * u, u * v, v * v};
    double sx = 0.0, sy = 0.0;
    for (int t = 0; t < 6; t++) { sx += b[t] * c[t]; sy += b[t] * c[6 + t]; }
    *X = sx; *Y = sy;
}

// rule 5: frame position -> sky
__device__ __forceinline__ void wcs_pix2sky(const wcs_geom& g, const double* c, double x, double y, double* ra, double* dec) {
    double X, Y;
    wcs_T(c, g.ny, g.nx, x, y, &X, &Y);
    const double xc = 0.5 * (double)(g.nx - 1), yc = 0.5 * (double)(g.ny - 1);
    const double dx = X - xc, dy = Y - yc;
    wcs_sky_of_std(g.cd[0] * dx + g.cd[1] * dy, g.cd[2] * dx + g.cd[3] * dy, g.ra0, g.dec0, ra, dec);
}

// ---------------------------------------------------------------------------------------------------------------------
// the catalogue as list B on the virtual grid
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WCS_BLOCK) void k_wcs_cat_list(int n, const double* __restrict__ sky, const float* __restrict__ mag, wcs_geom g,
                                                           double margin, double zp, int32_t* __restrict__ ys, int32_t* __restrict__ xs,
                                                           float* __restrict__ off, float* __restrict__ flux, float* __restrict__ err,
                                                           int32_t* __restrict__ count) {
    const int i = blockIdx.x * WCS_BLOCK + threadIdx.x;
    bool ok = false;
    if (i < n) {
        double xi, eta;
        const float m = mag[i];
        ok = wcs_std_of_sky(sky[2 * (size_t)i], sky[2 * (size_t)i + 1], g.ra0, g.dec0, &xi, &eta) && finite_f32(m);
        const double det = g.cd[0] * g.cd[3] - g.cd[1] * g.cd[2];
        const double x = 0.5 * (double)(g.nx - 1) + (g.cd[3] * xi - g.cd[1] * eta) / det;
        const double y = 0.5 * (double)(g.ny - 1) + (g.cd[0] * eta - g.cd[2] * xi) / det;
        ok = ok && x >= -margin && x <= (double)(g.nx - 1) + margin && y >= -margin && y <= (double)(g.ny - 1) + margin;
        const float f = ok ? (float)pow(10.0, -0.4 * ((double)m - zp)) : 0.f;
        ok = ok && f > 0.f && finite_f32(f);
        const float nanf_ = __builtin_nanf("");
        if (ok) {
            const double fx = floor(x + 0.5), fy = floor(y + 0.5);
            ys[i] = (int32_t)fy; xs[i] = (int32_t)fx;
            off[2 * (size_t)i] = (float)(y - fy); off[2 * (size_t)i + 1] = (float)(x - fx);
            flux[i] = f; err[i] = f / 1000.f;
        } else {
            ys[i] = 0; xs[i] = 0;
            off[2 * (size_t)i] = nanf_; off[2 * (size_t)i + 1] = nanf_;
            flux[i] = 0.f; err[i] = 0.f;
        }
    }
    const int c = wave_sum_i32(ok ? 1 : 0);                           // (every lane of the wave is here)
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, c);
}

static bool wcs_geom_ok(int ny, int nx, const double* cd, double ra0, double dec0) {
    if (ny < 1 || nx < 1 || !cd) return false;
    for (int k = 0; k < 4; k++)
        if (!std::isfinite(cd[k])) return false;
    const double det = cd[0] * cd[3] - cd[1] * cd[2];
    return det != 0.0 && std::isfinite(ra0) && std::isfinite(dec0) && fabs(dec0) <= 90.0;
}

extern "C" int bbx_wcs_cat_list(bbx_ctx* ctx, int n, const double* d_sky, const float* d_mag, double ra0, double dec0, int ny, int nx,
                                const double* cd, double margin, double mag_zp, int32_t* d_ys, int32_t* d_xs, float* d_off, float* d_flux,
                                float* d_err, int32_t* d_count, void* stream) {
    if (!ctx || n < 0 || !d_count || !wcs_geom_ok(ny, nx, cd, ra0, dec0) || !(margin >= 0.0) || !(margin < 1e9) || !std::isfinite(mag_zp))
        return BBX_ERR_ARG;
    if (n > 0 && (!d_sky || !d_mag || !d_ys || !d_xs || !d_off || !d_flux || !d_err)) return BBX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    BBX_HIP(hipMemsetAsync(d_count, 0, sizeof(int32_t), s));
    if (n == 0) return BBX_OK;
    wcs_geom g;
    for (int k = 0; k < 4; k++) g.cd[k] = cd[k];
    g.ra0 = ra0; g.dec0 = dec0; g.ny = ny; g.nx = nx;
    hipLaunchKernelGGL(k_wcs_cat_list, dim3((n + WCS_BLOCK - 1) / WCS_BLOCK), dim3(WCS_BLOCK), 0, s, n, d_sky, d_mag, g, margin, mag_zp, d_ys,
                       d_xs, d_off, d_flux, d_err, d_count);
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// pixel to sky
// ---------------------------------------------------------------------------------------------------------------------
// the position of row i: d_pos (x, y), else integer + offset (no offsets: the integer)
__device__ __forceinline__ void wcs_position(int i, const double* pos, const int32_t* ys, const int32_t* xs, const float* off, double* x, double* y) {
    if (pos) { *x = pos[2 * (size_t)i]; *y = pos[2 * (size_t)i + 1]; return; }
    *x = (double)xs[i] + (off ? (double)off[2 * (size_t)i + 1] : 0.0);
    *y = (double)ys[i] + (off ? (double)off[2 * (size_t)i] : 0.0);
}

__global__ __launch_bounds__(WCS_BLOCK) void k_wcs_pix2sky(int n, const double* __restrict__ pos, const int32_t* __restrict__ ys,
                                                          const int32_t* __restrict__ xs, const float* __restrict__ off,
                                                          const double* __restrict__ coef, wcs_geom g, double* __restrict__ sky) {
    const int i = blockIdx.x * WCS_BLOCK + threadIdx.x;
    if (i >= n) return;
    double c[12];
    for (int k = 0; k < 12; k++) c[k] = coef[k];
    double x, y, ra, dec;
    wcs_position(i, pos, ys, xs, off, &x, &y);
    wcs_pix2sky(g, c, x, y, &ra, &dec);
    sky[2 * (size_t)i] = ra; sky[2 * (size_t)i + 1] = dec;
}

extern "C" int bbx_wcs_pix2sky(bbx_ctx* ctx, int n, const double* d_pos, const int32_t* d_ys, const int32_t* d_xs, const float* d_off,
                               const double* d_coef, int ny, int nx, const double* cd, double ra0, double dec0, double* d_sky, void* stream) {
    if (!ctx || n < 0 || !wcs_geom_ok(ny, nx, cd, ra0, dec0)) return BBX_ERR_ARG;
    if (n == 0) return BBX_OK;
    if (!d_coef || !d_sky || (!d_pos && (!d_ys || !d_xs))) return BBX_ERR_ARG;
    wcs_geom g;
    for (int k = 0; k < 4; k++) g.cd[k] = cd[k];
    g.ra0 = ra0; g.dec0 = dec0; g.ny = ny; g.nx = nx;
    hipLaunchKernelGGL(k_wcs_pix2sky, dim3((n + WCS_BLOCK - 1) / WCS_BLOCK), dim3(WCS_BLOCK), 0, (hipStream_t)stream, n, d_pos, d_ys, d_xs,
                       d_off, d_coef, g, d_sky);
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// residuals of the pairs the last fit kept
// ---------------------------------------------------------------------------------------------------------------------
struct wcs_pairs {
    int n_items; const int32_t* items; const uint8_t* kept;
    int n_a; const int32_t* ys; const int32_t* xs; const float* off;
    int n_b; const double* cat;
    const double* coef;
    double* out;
};

// item i: (d_ra cos dec_cat, d_dec) [arcsec]; false: not a kept pair
__device__ __forceinline__ bool wcs_pair(const wcs_pairs& a, const wcs_geom& g, const double* c, int i, double* dra, double* ddec) {
    if (!a.kept[i]) return false;
    const int ia = a.items[2 * (size_t)i], ib = a.items[2 * (size_t)i + 1];
    if (ia < 0 || ib < 0 || ia >= a.n_a || ib >= a.n_b) return false;
    double x, y, ra, dec;
    wcs_position(ia, nullptr, a.ys, a.xs, a.off, &x, &y);
    wcs_pix2sky(g, c, x, y, &ra, &dec);
    const double rc = a.cat[2 * (size_t)ib], dc = a.cat[2 * (size_t)ib + 1];
    double d = ra - rc;
    d = d - 360.0 * floor((d + 180.0) / 360.0);                      // into [-180, 180)
    *dra = d * cos(dc * WCS_D2R) * 3600.0;
    *ddec = (dec - dc) * 3600.0;
    return true;
}

// the 256 per-thread values of v[k] added in thread order by thread 0, the totals to every thread
template <int N>
__device__ __forceinline__ void wcs_sum(double (&v)[N], double* s_part, double* s_tot) {
    __syncthreads();
    for (int k = 0; k < N; k++) s_part[k * WCS_BLOCK + threadIdx.x] = v[k];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 0; k < N; k++) {
            double t = 0.0;
            for (int j = 0; j < WCS_BLOCK; j++) t += s_part[k * WCS_BLOCK + j];
            s_tot[k] = t;
        }
    __syncthreads();
    for (int k = 0; k < N; k++) v[k] = s_tot[k];
}

__global__ __launch_bounds__(WCS_BLOCK) void k_wcs_pair_stats(wcs_pairs a, wcs_geom g) {
    __shared__ double s_part[3 * WCS_BLOCK];
    __shared__ double s_tot[3];
    double c[12];
    for (int k = 0; k < 12; k++) c[k] = a.coef[k];
    double p[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < a.n_items; i += WCS_BLOCK) {
        double dra, ddec;
        if (wcs_pair(a, g, c, i, &dra, &ddec)) { p[0] += 1.0; p[1] += dra; p[2] += ddec; }
    }
    wcs_sum<3>(p, s_part, s_tot);
    const double cnt = p[0], mra = p[1] / cnt, mdec = p[2] / cnt;     // (NaN for no pair)
    double q[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < a.n_items; i += WCS_BLOCK) {
        double dra, ddec;
        if (wcs_pair(a, g, c, i, &dra, &ddec)) { q[1] += (dra - mra) * (dra - mra); q[2] += (ddec - mdec) * (ddec - mdec); }
    }
    wcs_sum<3>(q, s_part, s_tot);
    if (threadIdx.x == 0) {
        a.out[0] = cnt; a.out[1] = mra; a.out[2] = sqrt(q[1] / cnt); a.out[3] = mdec; a.out[4] = sqrt(q[2] / cnt);
        a.out[5] = 0.0; a.out[6] = 0.0; a.out[7] = 0.0;
    }
}

extern "C" int bbx_wcs_pair_stats(bbx_ctx* ctx, int n_items, const int32_t* d_items, const uint8_t* d_kept, int n_a, const int32_t* d_a_ys,
                                  const int32_t* d_a_xs, const float* d_a_off, int n_b, const double* d_cat_sky, const double* d_coef, int ny,
                                  int nx, const double* cd, double ra0, double dec0, double* d_out, void* stream) {
    if (!ctx || n_items < 0 || n_a < 0 || n_b < 0 || !d_out || !wcs_geom_ok(ny, nx, cd, ra0, dec0)) return BBX_ERR_ARG;
    if (n_items > 0 && (!d_items || !d_kept || !d_coef)) return BBX_ERR_ARG;
    if (n_items > 0 && n_a > 0 && (!d_a_ys || !d_a_xs || !d_a_off)) return BBX_ERR_ARG;
    if (n_items > 0 && n_b > 0 && !d_cat_sky) return BBX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (n_items == 0) return BBX_OK;                                 // (d_out stays as the caller made it)
    wcs_pairs a;
    a.n_items = n_items; a.items = d_items; a.kept = d_kept; a.n_a = n_a; a.ys = d_a_ys; a.xs = d_a_xs; a.off = d_a_off;
    a.n_b = n_b; a.cat = d_cat_sky; a.coef = d_coef; a.out = d_out;
    wcs_geom g;
    for (int k = 0; k < 4; k++) g.cd[k] = cd[k];
    g.ra0 = ra0; g.dec0 = dec0; g.ny = ny; g.nx = nx;
    hipLaunchKernelGGL(k_wcs_pair_stats, dim3(1), dim3(WCS_BLOCK), 0, s, a, g);
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}
