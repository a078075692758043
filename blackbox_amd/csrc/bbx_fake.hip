// bbx_fake.hip -- fake stars (include/bbx.h, bbx_fake_inject / bbx_fake_recover): stars of an asked S/N are added
// to the background-subtracted new frame in place, just before it is cut into sub-images, and read back from Scorr / Fpsf /
// Fpsferr behind the subtraction.
//
//   k_fake_inject : one workgroup of 256 per star
//     1 stamp   step 1 of k_psf_optflux_shift (the model's fmaf chain or the plane d_idx picks), psb_shift_stamp by d_off,
//               the float64 sum (psb_stamp_sum)
//     2 rules   off the frame, a mask in the clear window, a source or a non-finite value there, no usable S/N or sigma: the
//               first that holds is the star's flag and the star adds nothing (uniform per workgroup)
//     3 flux    S/N(F)^2 = sum F^2 P^2 / (sigma^2 + F max(P, 0)) = s^2: convex and increasing in F, Newton from the upper
//               bracket kept inside [F_lo, F_hi], float64, every sum by wg_sum_seq
//     4 add     frame + F P [+ sqrt(F max(P, 0)) g] in float64, rounded to float32 once; g from Philox4x32-10 keyed on the seed,
//               counter (pixel, star): no state, no atomics.  Each pixel is read and written by one thread, and the caller keeps
//               the stamps of two stars apart, so the stores need no ordering among workgroups
//   k_fake_recover : one wave per star, the largest finite Scorr of the window by a wave reduction on (value, window index)
#include "bbx_spline.h"

#define FK_BLOCK 256
#define FK_SMAX  49
#define FK_NITER 100

struct fk_args {
    float* frame; const float* ref; const float* sigma; const uint8_t* mask_new; const uint8_t* mask_ref;
    const float* cube; const float* terms; const int32_t* idx;
    const int32_t* ys; const int32_t* xs; const float* off; const float* s2n;
    float* flux; float* real; float* snr_sky; uint8_t* flags;
    int ny, nx, S, nplane, clear_half, noise;
    float clear_nsigma;
    unsigned key0, key1;
};

// Philox4x32-10 (Salmon et al. 2011): counter c[4], key k[2] -> c[4]
__device__ __forceinline__ void fk_philox(unsigned c[4], unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1;
        c[1] = (unsigned)p1; c[3] = (unsigned)p0; c[0] = n0; c[2] = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}
// the standard normal of pixel k of star s: Box-Muller on the first two words, in float64
__device__ __forceinline__ double fk_normal(unsigned k, unsigned s, unsigned key0, unsigned key1) {
    unsigned c[4] = {k, s, 0u, 0u};
    fk_philox(c, key0, key1);
    const double u1 = ((double)c[0] + 0.5) * (1.0 / 4294967296.0), u2 = ((double)c[1] + 0.5) * (1.0 / 4294967296.0);
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

// the largest of v over the workgroup, the same in every thread (v >= 0; the order of a max does not reach its bits)
__device__ __forceinline__ double fk_wg_max(double v, double* red) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = red[0];
#pragma unroll
    for (int w = 1; w < FK_BLOCK / 64; w++) t = fmax(t, red[w]);
    return t;
}

template <bool MINI>
__global__ __launch_bounds__(FK_BLOCK) void k_fake_inject(fk_args a, bbx_spl sp) {
    __shared__ float s_a[FK_SMAX * FK_SMAX];                         // the stamp
    __shared__ float s_b[FK_SMAX * FK_SMAX];                         // the row pass's output, then sigma at the stamp's pixels
    __shared__ double s_red[2 * (FK_BLOCK / 64)];
    const int tid = threadIdx.x, s = blockIdx.x;
    const int S = a.S, npx = S * S, h = S / 2;
    // ---- 1: the stamp, shifted, and its sum
    if (a.terms) {
        const float* t = a.terms + (size_t)s * a.nplane;
        for (int k = tid; k < npx; k += FK_BLOCK) {
            float m = 0.f;
            for (int kk = 0; kk < a.nplane; kk++) m = __builtin_fmaf(t[kk], a.cube[(size_t)kk * npx + k], m);
            s_a[k] = m;
        }
    } else {
        const int pl = min(max(a.idx[s], 0), a.nplane - 1);
        const float* p = a.cube + (size_t)pl * npx;
        for (int k = tid; k < npx; k += FK_BLOCK) s_a[k] = p[k];
    }
    const float dy = a.off[2 * (size_t)s], dx = a.off[2 * (size_t)s + 1];
    const bool cen = fabsf(dy) <= 0.5f && fabsf(dx) <= 0.5f;         // (uniform; false for a NaN)
    __syncthreads();
    if (cen) psb_shift_stamp<FK_BLOCK>(s_a, s_b, S, dy, dx);
    const double norm = psb_stamp_sum<FK_BLOCK>(s_a, npx, s_red);
    // ---- 2: the rules, in their order of precedence
    unsigned fl = 0u;
    const long long yc = a.ys[s], xc = a.xs[s];
    const long long y0 = yc - h, x0 = xc - h;
    if (!(cen && norm > 0.0 && norm < 1.0e300)) fl = 8u;
    else if (y0 < 0 || x0 < 0 || y0 + S > a.ny || x0 + S > a.nx) fl = 4u;
    if (!fl) {
        // the clear window, clipped to the frame (clear_half <= S / 2: it lies inside this star's own stamp)
        const int W = 2 * a.clear_half + 1;
        int masked = 0, source = 0;
        for (int k = tid; k < W * W; k += FK_BLOCK) {
            const int r = k / W, c = k - r * W;
            const long long y = yc - a.clear_half + r, x = xc - a.clear_half + c;
            if (y < 0 || y >= a.ny || x < 0 || x >= a.nx) continue;
            const size_t ix = (size_t)y * a.nx + (size_t)x;
            if ((a.mask_new && a.mask_new[ix]) || (a.mask_ref && a.mask_ref[ix])) masked = 1;
            const float sg = MINI ? bbx_spl_eval(sp, (int)y, (int)x) : a.sigma[ix];
            const float lim = a.clear_nsigma * sg;
            const float d = a.frame[ix];
            if (!finite_f32(d) || fabsf(d) > lim) source = 1;
            if (a.ref) {
                const float rv = a.ref[ix];
                if (!finite_f32(rv) || fabsf(rv) > lim) source = 1;
            }
        }
        const int any_masked = __syncthreads_or(masked), any_source = __syncthreads_or(source);
        if (any_masked) fl = 1u;
        else if (any_source) fl = 2u;
    }
    double F = 0.0, A = 0.0;
    if (!fl) {
        // sigma at the stamp's pixels, A = sum P^2 / sigma^2, q = max(max(P, 0) / sigma^2)
        int bad = 0;
        double pa = 0.0, pq = 0.0;
        for (int k = tid; k < npx; k += FK_BLOCK) {
            const int r = k / S, c = k - r * S;
            const float sg = MINI ? bbx_spl_eval(sp, (int)(y0 + r), (int)(x0 + c)) : a.sigma[(size_t)(y0 + r) * a.nx + (size_t)(x0 + c)];
            s_b[k] = sg;
            if (!(sg > 0.f) || !finite_f32(sg)) { bad = 1; continue; }
            const double v = (double)(sg * sg), p = (double)s_a[k] / norm;
            if (!(v > 0.0)) { bad = 1; continue; }                    // (a sigma whose square underflows)
            pa += p * p / v;
            pq = fmax(pq, fmax(p, 0.0) / v);
        }
        const float sn = a.s2n[s];
        if (__syncthreads_or(bad) || !(sn > 0.f) || !finite_f32(sn)) fl = 16u;
        else {
            A = wg_sum_seq<FK_BLOCK / 64>(pa, s_red);
            const double q = fk_wg_max(pq, s_red);
            if (!(A > 0.0 && A < 1.0e300 && q < 1.0e300)) fl = 16u;
            else {
                // ---- 3: the flux of the asked S/N
                const double s2 = (double)sn * (double)sn;
                double lo = (double)sn / sqrt(A), hi = (s2 * q + sqrt(s2 * s2 * q * q + 4.0 * A * s2)) / (2.0 * A);
                F = hi;
                for (int it = 0; it < FK_NITER; it++) {              // (uniform: every thread holds the same sums)
                    double hv[2] = {0.0, 0.0};
                    for (int k = tid; k < npx; k += FK_BLOCK) {
                        const double v = (double)(s_b[k] * s_b[k]), p = (double)s_a[k] / norm;
                        const double pp = fmax(p, 0.0), w = v + F * pp, fp2 = F * p * p;
                        hv[0] += F * fp2 / w;
                        hv[1] += fp2 * (2.0 * v + F * pp) / (w * w);
                    }
                    wg_sum_seq<FK_BLOCK / 64, 2>(hv, s_red);
                    const double g = hv[0] - s2;
                    if (g == 0.0) break;                             // (on the root)
                    if (g > 0.0) hi = F; else lo = F;
                    double Fn = F - g / hv[1];
                    if (Fn == F) break;                              // (the step is below one ulp: no bisection away from the root)
                    if (!(Fn > lo && Fn < hi)) Fn = 0.5 * (lo + hi);
                    const bool done = fabs(Fn - F) <= 1.0e-15 * fabs(Fn) || !(hi > lo);
                    F = Fn;
                    if (done) break;
                }
                if (!(F > 0.0 && F < 3.0e38)) fl = 16u;
            }
        }
    }
    // ---- 4: the star
    double tot = 0.0;
    const float Ff = fl ? 0.f : (float)F;
    if (!fl) {
        const double Fd = (double)Ff;
        for (int k = tid; k < npx; k += FK_BLOCK) {
            const int r = k / S, c = k - r * S;
            const size_t ix = (size_t)(y0 + r) * a.nx + (size_t)(x0 + c);
            const double p = (double)s_a[k] / norm;
            double add = Fd * p;
            if (a.noise) add += sqrt(Fd * fmax(p, 0.0)) * fk_normal((unsigned)k, (unsigned)s, a.key0, a.key1);
            a.frame[ix] = (float)((double)a.frame[ix] + add);
            tot += add;
        }
    }
    tot = wg_sum_seq<FK_BLOCK / 64>(tot, s_red);
    // ---- 5: the star's row
    if (tid == 0) {
        a.flux[s] = Ff;
        a.real[s] = fl ? 0.f : (float)tot;
        a.snr_sky[s] = fl ? 0.f : (float)((double)Ff * sqrt(A));
        a.flags[s] = (uint8_t)fl;
    }
}

extern "C" int bbx_fake_inject(bbx_ctx* ctx, int ny, int nx, float* d_frame, const float* d_ref, const float* d_sigma,
                               const bbx_spline_image* sigma_mini, const uint8_t* d_mask_new, const uint8_t* d_mask_ref, int S, int nplane,
                               const float* d_cube, const float* d_terms, const int32_t* d_idx, int nstar, const int32_t* d_ys,
                               const int32_t* d_xs, const float* d_off, const float* d_s2n, int clear_half, float clear_nsigma, int noise,
                               uint64_t seed, float* d_flux, float* d_real, float* d_snr_sky, uint8_t* d_flags, void* stream) {
    if (!ctx || ny < 1 || nx < 1 || S < 1 || S > FK_SMAX || !(S & 1) || nplane < 1 || nstar < 0) return BBX_ERR_ARG;
    if ((d_terms != nullptr) == (d_idx != nullptr) || (d_sigma != nullptr) == (sigma_mini != nullptr)) return BBX_ERR_ARG;      // one form each
    if (d_terms && nplane > 64) return BBX_ERR_ARG;
    if (clear_half < 0 || clear_half > S / 2 || !(clear_nsigma >= 0.f) || (noise != 0 && noise != 1)) return BBX_ERR_ARG;
    bbx_spl sp = {};
    if (sigma_mini) {
        const int rc = bbx_spl_make(sigma_mini, ny, nx, &sp);
        if (rc) return rc;
    }
    if (nstar == 0) return BBX_OK;
    if (!d_frame || !d_cube || !d_ys || !d_xs || !d_off || !d_s2n || !d_flux || !d_real || !d_snr_sky || !d_flags) return BBX_ERR_ARG;
    const fk_args a = {d_frame, d_ref, d_sigma, d_mask_new, d_mask_ref, d_cube, d_terms, d_idx, d_ys, d_xs, d_off, d_s2n,
                       d_flux, d_real, d_snr_sky, d_flags, ny, nx, S, nplane, clear_half, noise, clear_nsigma,
                       (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32)};
    if (sigma_mini)
        hipLaunchKernelGGL(k_fake_inject<true>, dim3(nstar), dim3(FK_BLOCK), 0, (hipStream_t)stream, a, sp);
    else
        hipLaunchKernelGGL(k_fake_inject<false>, dim3(nstar), dim3(FK_BLOCK), 0, (hipStream_t)stream, a, sp);
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}

// ---- the stars read back: one wave per star
__global__ __launch_bounds__(FK_BLOCK) void k_fake_recover(const float* __restrict__ scorr, const float* __restrict__ fpsf,
                                                           const float* __restrict__ fpsferr, const int32_t* __restrict__ ys,
                                                           const int32_t* __restrict__ xs, int ny, int nx, int nstar, int radius,
                                                           float* __restrict__ out) {
    const int lane = threadIdx.x & 63, s = (int)blockIdx.x * (FK_BLOCK / 64) + (threadIdx.x >> 6);
    if (s >= nstar) return;                                          // (whole waves: no barrier below)
    const long long yc = ys[s], xc = xs[s];
    const int W = 2 * radius + 1;
    float best = 0.f;
    int bi = 0x7fffffff;                                             // window index of the best pixel; none yet
    for (int k = lane; k < W * W; k += 64) {                         // ascending: a tie inside a lane keeps the lower index
        const int r = k / W, c = k - r * W;
        const long long y = yc - radius + r, x = xc - radius + c;
        if (y < 0 || y >= ny || x < 0 || x >= nx) continue;
        const float v = scorr[(size_t)y * nx + (size_t)x];
        if (!finite_f32(v)) continue;
        if (bi == 0x7fffffff || v > best) { best = v; bi = k; }
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const float ov = __shfl_xor(best, m, 64);
        const int oi = __shfl_xor(bi, m, 64);
        if (oi != 0x7fffffff && (bi == 0x7fffffff || ov > best || (ov == best && oi < bi))) { best = ov; bi = oi; }
    }
    if (lane == 0) {
        float* o = out + (size_t)s * 6;
        const bool in = yc >= 0 && yc < ny && xc >= 0 && xc < nx;
        const float at = in ? fpsf[(size_t)yc * nx + (size_t)xc] : 0.f;
        if (bi == 0x7fffffff) {
            const float nan = __uint_as_float(0x7fc00000u);
            o[0] = nan; o[1] = nan; o[2] = 0.f; o[3] = 0.f; o[4] = 0.f; o[5] = 0.f;
        } else {
            const int r = bi / W, c = bi - r * W;
            const size_t ix = (size_t)(yc - radius + r) * nx + (size_t)(xc - radius + c);
            o[0] = (float)(r - radius); o[1] = (float)(c - radius); o[2] = best; o[3] = fpsf[ix]; o[4] = fpsferr[ix]; o[5] = at;
        }
    }
}

extern "C" int bbx_fake_recover(bbx_ctx* ctx, int ny, int nx, const float* d_scorr, const float* d_fpsf, const float* d_fpsferr, int nstar,
                                const int32_t* d_ys, const int32_t* d_xs, int radius, float* d_out, void* stream) {
    if (!ctx || ny < 1 || nx < 1 || nstar < 0 || radius < 0 || radius > 4) return BBX_ERR_ARG;
    if (nstar == 0) return BBX_OK;
    if (!d_scorr || !d_fpsf || !d_fpsferr || !d_ys || !d_xs || !d_out) return BBX_ERR_ARG;
    const int per = FK_BLOCK / 64;
    hipLaunchKernelGGL(k_fake_recover, dim3((nstar + per - 1) / per), dim3(FK_BLOCK), 0, (hipStream_t)stream, d_scorr, d_fpsf, d_fpsferr, d_ys, d_xs,
                       ny, nx, nstar, radius, d_out);
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}
