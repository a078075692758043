// bbx_psfphot.hip -- catalogue photometry with the PSF placed on the source's centroid (include/bbx.h, bbx_psf_optflux_shift;
// DESIGN.md 4h): per source the PSF stamp is formed, shifted by the centroid offset, normalised and folded with the frame in
// one workgroup; the stamp lives in LDS only, two floats and a byte per source leave the chip.
//
//   k_psf_optflux_shift : one workgroup of 256 per source
//     1 stamp   lane = stamp pixel: the PSFEx model's k-ordered float32 fmaf chain (k_psf_model's arithmetic; the basis reads
//               coalesce, the cube of <= 64 planes stays in L2), or a copy of the plane d_idx[s] picks
//     2 shift   LANCZOS3, separable: row pass (along x) into the second buffer, column pass back (psb_shift_stamp, bbx_common.h)
//     3 norm    sum of the S x S pixels in float64 (psb_stamp_sum)
//     4 sums    num = sum P D / V, den = sum P^2 / V in float64, V = max(D, 0) + sigma^2 in float32 (k_variance's)
//   Block sums: per-thread partial sums over pixels tid, tid + 256, ..., the waves' totals through LDS in wave order
//   (wg_sum_seq): no atomics, the same input gives the same bits.
#include "bbx_spline.h"

#define PPH_BLOCK  256
#define PPH_SMAX   49
#define PPH_OFFMAX 16.f
#define PPH_KI     4                                                 // coefficient columns of the sigma mini image a stamp may cross (k_psf_optflux_mini's)

struct pph_args {
    const float* D; const float* sigma; const uint8_t* mask;
    const float* cube; const float* terms; const int32_t* idx;
    const int32_t* ys; const int32_t* xs; const float* off;
    float* flux; float* err; uint8_t* flags;
    int ny, nx, S, nplane;
};

template <bool MINI>
__global__ __launch_bounds__(PPH_BLOCK) void k_psf_optflux_shift(pph_args a, bbx_spl sp) {
    __shared__ float s_a[PPH_SMAX * PPH_SMAX];                       // 9.6 KB each: the stamp, and the row pass's output
    __shared__ float s_b[PPH_SMAX * PPH_SMAX];
    __shared__ double s_red[PPH_BLOCK / 64];
    // sigma off the mini image, as k_psf_optflux_mini reads it: which coefficient column each stamp column lies in and its place t
    // inside, the cubics of the stamp's rows on those columns (bbx_spl_poly: S x nk of them instead of S^2), one Horner per pixel
    __shared__ float4 s_poly[MINI ? PPH_SMAX : 1][PPH_KI];
    __shared__ float s_t[MINI ? PPH_SMAX : 1];
    __shared__ int s_k[MINI ? PPH_SMAX : 1], s_c[PPH_KI], s_nk;
    const int tid = threadIdx.x, s = blockIdx.x;
    const int S = a.S, npx = S * S, h = S / 2;
    // ---- 1: the stamp
    if (a.terms) {
        const float* t = a.terms + (size_t)s * a.nplane;             // (uniform per workgroup: scalar loads)
        for (int k = tid; k < npx; k += PPH_BLOCK) {
            float m = 0.f;
            for (int kk = 0; kk < a.nplane; kk++) m = __builtin_fmaf(t[kk], a.cube[(size_t)kk * npx + k], m);
            s_a[k] = m;
        }
    } else {
        const int pl = min(max(a.idx[s], 0), a.nplane - 1);
        const float* p = a.cube + (size_t)pl * npx;
        for (int k = tid; k < npx; k += PPH_BLOCK) s_a[k] = p[k];
    }
    // ---- 2: to the centroid
    const float dy = a.off[2 * (size_t)s], dx = a.off[2 * (size_t)s + 1];
    const bool cen = finite_f32(dy) && finite_f32(dx) && fabsf(dy) <= PPH_OFFMAX && fabsf(dx) <= PPH_OFFMAX;      // (uniform)
    unsigned fl = cen ? 0u : 1u;
    __syncthreads();
    if (cen) psb_shift_stamp<PPH_BLOCK>(s_a, s_b, S, dy, dx);
    // ---- 3: unit sum
    const double norm = psb_stamp_sum<PPH_BLOCK>(s_a, npx, s_red);
    const bool ok = norm > 0.0 && norm < 1.0e300;                    // (uniform: every thread holds the same norm)
    if (!ok) fl |= 4u;
    // ---- 4: the two sums
    double num = 0.0, den = 0.0;
    int hit = 0;
    const long long y0 = (long long)a.ys[s] - h, x0 = (long long)a.xs[s] - h;
    bool fits = false;
    if (MINI && ok) {
        if (tid < 64) {                                              // (wave 0; S <= 49 columns)
            int c = 0, r = 0;
            const int X = (int)min(max(x0 + tid, 0ll), (long long)a.nx - 1);
            bbx_spl_axis(X, sp.pw, sp.rpw, sp.px, sp.npad, sp.nx1, sp.dx, sp.rdx, c, r);
            const int cprev = __shfl_up(c, 1, 64);
            const bool act = tid < S;
            const unsigned long long chg = __ballot(act && tid > 0 && c != cprev);
            const int kk = __popcll(chg & ((2ull << tid) - 1ull));   // changes at lanes <= this one
            const int nk = __popcll(chg) + 1;
            if (act) { s_k[tid] = kk; s_t[tid] = (float)r * sp.rdx; }
            if (nk <= PPH_KI && act && (tid == 0 || ((chg >> tid) & 1ull))) s_c[kk] = c;
            if (tid == 0) s_nk = nk;
        }
        __syncthreads();
        const int nk = s_nk;
        fits = nk <= PPH_KI;                                         // (uniform; otherwise every pixel evaluates the spline itself)
        if (fits) {
            for (int t = tid; t < S * nk; t += PPH_BLOCK) {
                const int j = t / nk, q = t - j * nk;
                const int Y = (int)min(max(y0 + j, 0ll), (long long)a.ny - 1);
                s_poly[j][q] = bbx_spl_poly(sp, Y, s_c[q]);
            }
        }
        __syncthreads();
    }
    if (ok) {
        for (int k = tid; k < npx; k += PPH_BLOCK) {
            const int r = k / S, c = k - r * S;
            const long long y = y0 + r, x = x0 + c;
            if (y < 0 || y >= a.ny || x < 0 || x >= a.nx) continue;
            const size_t ix = (size_t)y * a.nx + (size_t)x;
            if (a.mask && a.mask[ix]) { hit = 1; continue; }
            const float d = a.D[ix];
            if (!finite_f32(d)) continue;
            float sg;
            if (!MINI) sg = a.sigma[ix];
            else if (fits) sg = bbx_spl_horner(s_poly[r][s_k[c]], s_t[c]);
            else sg = bbx_spl_eval(sp, (int)y, (int)x);
            const double v = (double)(fmaxf(d, 0.f) + sg * sg);
            if (!(v > 0.0)) continue;
            const double p = (double)s_a[k] / norm;
            num += p * (double)d / v;
            den += p * p / v;
        }
    }
    if (__syncthreads_or(hit)) fl |= 2u;
    num = wg_sum_seq<PPH_BLOCK / 64>(num, s_red);
    den = wg_sum_seq<PPH_BLOCK / 64>(den, s_red);
    if (tid == 0) {
        a.flux[s] = den > 0.0 ? (float)(num / den) : 0.f;
        a.err[s] = den > 0.0 ? (float)(1.0 / sqrt(den)) : 0.f;
        a.flags[s] = (uint8_t)fl;
    }
}

extern "C" int bbx_psf_optflux_shift(bbx_ctx* ctx, int ny, int nx, const float* d_D, const float* d_sigma, const bbx_spline_image* sigma_mini,
                                     const uint8_t* d_mask, int S, int nplane, const float* d_cube, const float* d_terms, const int32_t* d_idx,
                                     int nsrc, const int32_t* d_ys, const int32_t* d_xs, const float* d_off, float* d_flux, float* d_err,
                                     uint8_t* d_flags, void* stream) {
    if (!ctx || ny < 1 || nx < 1 || S < 1 || S > PPH_SMAX || !(S & 1) || nplane < 1 || nsrc < 0) return BBX_ERR_ARG;
    if ((d_terms != nullptr) == (d_idx != nullptr) || (d_sigma != nullptr) == (sigma_mini != nullptr)) return BBX_ERR_ARG;      // one form each
    if (d_terms && nplane > 64) return BBX_ERR_ARG;
    bbx_spl sp = {};
    if (sigma_mini) {
        const int rc = bbx_spl_make(sigma_mini, ny, nx, &sp);
        if (rc) return rc;
    }
    if (nsrc == 0) return BBX_OK;
    if (!d_D || !d_cube || !d_ys || !d_xs || !d_off || !d_flux || !d_err || !d_flags) return BBX_ERR_ARG;
    const pph_args a = {d_D, d_sigma, d_mask, d_cube, d_terms, d_idx, d_ys, d_xs, d_off, d_flux, d_err, d_flags, ny, nx, S, nplane};
    if (sigma_mini)
        hipLaunchKernelGGL(k_psf_optflux_shift<true>, dim3(nsrc), dim3(PPH_BLOCK), 0, (hipStream_t)stream, a, sp);
    else
        hipLaunchKernelGGL(k_psf_optflux_shift<false>, dim3(nsrc), dim3(PPH_BLOCK), 0, (hipStream_t)stream, a, sp);
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}
