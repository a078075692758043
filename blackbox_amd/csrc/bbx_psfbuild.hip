// bbx_psfbuild.hip -- a PSF model from the frame's own stars: a PSFEx-style polynomial pixel basis (the form bbx_psf_model
// evaluates and fitsio.read_psfex reads).  [EXT] PSFEx is not in the reference tree: the rules here are THIS PROJECT'S OWN
// (include/bbx.h), parity with PSFEx's numbers is unpinned.
//
//   k_psf_reason  : one thread per source: the selection rules, the isolation rule by the band search of k_match_nearest
//   k_psf_compact : one workgroup: count, stride, compaction in list order (the walk of bbx_stats.h; no atomics)
//   k_psf_stamps  : one workgroup per star: window in LDS, LANCZOS3 row pass, column pass, norm, weights
//   k_psf_fit     : lane = vignette pixel, the stars split over the waves of a workgroup, the partial normal equations
//                   combined through LDS in wave order, Cholesky in float64 per lane
//   k_psf_chi2    : one workgroup per star
// Every sum runs in a fixed order: the same input gives the same bits.
#include "bbx_stats.h"

#define PSB_BLOCK     256
#define PSB_VMAX      49
#define PSB_WMAX      (PSB_VMAX + 5)                     // window side: the vignette and its six taps
#define PSB_FIT_BLOCK 512
#define PSB_FIT_WAVES (PSB_FIT_BLOCK / 64)
#define PSB_NCOEF_MAX 10                                 // poldeg <= 3
#define PSB_PD_EPS    1e-13                              // a pivot below this fraction of its diagonal element: not positive definite

// ---------------------------------------------------------------------------------------------------------------------
// selection
// ---------------------------------------------------------------------------------------------------------------------
struct psf_sel_in {
    const int32_t* ys; const int32_t* xs; const float* pk; const float* shapes; const uint8_t* flags;
    const double* d_fwhm_med;
    int n, ny, nx, V;
    float sigma_bkg, snr_min, fwhm_med, fwhm_tol, elong_max, iso_frac;
};

__global__ __launch_bounds__(PSB_BLOCK) void k_psf_reason(psf_sel_in in, uint8_t* __restrict__ reason) {
    const int i = blockIdx.x * PSB_BLOCK + threadIdx.x;
    if (i >= in.n) return;
    const float* sh = in.shapes + 8 * (size_t)i;
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 8; k++) fin = fin && finite_f32(sh[k]);
    const float pk = in.pk[i];
    const float fmed = in.d_fwhm_med ? (float)in.d_fwhm_med[0] : in.fwhm_med;
    const int y = in.ys[i], x = in.xs[i], h = in.V / 2, m = h + 3;
    int r = 0;
    if (!fin || in.flags[i] != 0) r = 1;
    else if (!(pk / in.sigma_bkg >= in.snr_min)) r = 2;
    else if (!(fabsf(sh[5] / fmed - 1.0f) <= in.fwhm_tol) || !(sh[6] <= in.elong_max)) r = 3;
    else if (y < m || y > in.ny - 1 - m || x < m || x > in.nx - 1 - m) r = 4;
    else {
        const float lim = in.iso_frac * pk;
        for (int j = match_lower_bound(in.ys, in.n, y - h); j < in.n; j++) {
            const int yj = in.ys[j];
            if (yj > y + h) break;
            const int xj = in.xs[j];
            if (j == i || xj < x - h || xj > x + h) continue;
            if (in.pk[j] > lim) { r = 5; break; }
        }
    }
    reason[i] = (uint8_t)r;
}

struct psf_sel_item {
    const uint8_t* __restrict__ reason;
    int32_t* __restrict__ star;
    __device__ __forceinline__ bool load(int i, const stats_seg&) { return reason[i] == 0; }
    __device__ __forceinline__ void put(int i, int pos) { star[pos] = i; }
};

__global__ __launch_bounds__(STATS_BLOCK) void k_psf_compact(int n, const uint8_t* __restrict__ reason, int cap, int32_t* __restrict__ star,
                                                             int32_t* __restrict__ nstar) {
    __shared__ int s_cnt[STATS_WAVES];
    stats_seg sg = {0, n, INT32_MIN, INT32_MAX, INT32_MIN, INT32_MAX, 1};
    psf_sel_item it = {reason, star};
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int mine = stats_walk<true>(sg, 0, it);
    if (lane == 0) s_cnt[wave] = mine;
    __syncthreads();
    int nq = 0, base = 0;
#pragma unroll
    for (int w = 0; w < STATS_WAVES; w++) { if (w < wave) base += s_cnt[w]; nq += s_cnt[w]; }
    sg.stride = nq > cap ? (nq + cap - 1) / cap : 1;                  // (the kept ones: ceil(nq / stride) <= cap <= BBX_MATCH_CAP)
    stats_walk<false>(sg, base, it);
    if (threadIdx.x == 0) { nstar[0] = nq; nstar[1] = sg.stride; }
}

extern "C" int bbx_psf_select(bbx_ctx* ctx, int n, const int32_t* d_ys, const int32_t* d_xs, const float* d_pk, const float* d_shapes,
                              const uint8_t* d_flags, float sigma_bkg, float snr_min, float fwhm_med, const double* d_fwhm_med,
                              float fwhm_tol, float elong_max, float iso_frac, int V, int ny, int nx, int cap, uint8_t* d_reason,
                              int32_t* d_star, int32_t* d_nstar, void* stream) {
    if (!ctx || n < 0 || V < 1 || V > PSB_VMAX || !(V & 1) || ny < 1 || nx < 1 || cap < 1 || cap > BBX_MATCH_CAP || !d_nstar ||
        !(sigma_bkg > 0.f) || !(fwhm_tol >= 0.f) || !(iso_frac >= 0.f))
        return BBX_ERR_ARG;
    if (n > 0 && (!d_ys || !d_xs || !d_pk || !d_shapes || !d_flags || !d_reason || !d_star)) return BBX_ERR_ARG;
    if (n > 0) {
        const psf_sel_in in = {d_ys, d_xs, d_pk, d_shapes, d_flags, d_fwhm_med, n, ny, nx, V, sigma_bkg, snr_min, fwhm_med, fwhm_tol,
                               elong_max, iso_frac};
        hipLaunchKernelGGL(k_psf_reason, dim3((n + PSB_BLOCK - 1) / PSB_BLOCK), dim3(PSB_BLOCK), 0, (hipStream_t)stream, in, d_reason);
        BBX_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_psf_compact, dim3(1), dim3(STATS_BLOCK), 0, (hipStream_t)stream, n, d_reason, cap, d_star, d_nstar);
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// vignettes
// ---------------------------------------------------------------------------------------------------------------------
// (wg_sum_seq, psb_taps: bbx_common.h -- bbx_psfphot.hip shifts its stamps with the same taps)
__global__ __launch_bounds__(PSB_BLOCK) void k_psf_stamps(int ny, int nx, const float* __restrict__ img, const uint8_t* __restrict__ mask,
                                                          int nsrc, const int32_t* __restrict__ ys, const int32_t* __restrict__ xs,
                                                          const float* __restrict__ shapes, const float* __restrict__ sig,
                                                          const int32_t* __restrict__ star, const int32_t* __restrict__ nstar_dev, int V,
                                                          float acc, float* __restrict__ out_I, float* __restrict__ out_w,
                                                          double* __restrict__ out_norm, uint8_t* __restrict__ out_ok) {
    __shared__ float s_win[PSB_WMAX * PSB_WMAX];                     // 11.7 KB
    __shared__ float s_row[PSB_WMAX * PSB_VMAX];                     // row pass: [V + 5][V]
    __shared__ float s_st[PSB_VMAX * PSB_VMAX];
    __shared__ double s_red[PSB_BLOCK / 64];
    const int tid = threadIdx.x, s = blockIdx.x;
    const int W = V + 5, h = V / 2, npx = V * V;
    float* oI = out_I + (size_t)s * npx;
    float* ow = out_w + (size_t)s * npx;
    // ---- which source, where (uniform per workgroup)
    bool live = true;
    if (nstar_dev) {
        const int nq = nstar_dev[0], st = nstar_dev[1];
        live = st >= 1 && s < (nq + st - 1) / st;
    }
    int src = 0;
    if (live) src = star ? star[s] : s;
    live = live && src >= 0 && src < nsrc;
    int y0 = 0, x0 = 0;
    float fy = 0.f, fx = 0.f, sg = 0.f;
    if (live) {
        const float cy = shapes[8 * (size_t)src], cx = shapes[8 * (size_t)src + 1];
        sg = sig[src];
        live = finite_f32(cy) && finite_f32(cx) && fabsf(cy) <= 16.f && fabsf(cx) <= 16.f && finite_f32(sg);
        if (live) {
            const float ly = floorf(cy), lx = floorf(cx);
            fy = cy - ly; fx = cx - lx;
            y0 = ys[src] + (int)ly - h - 2; x0 = xs[src] + (int)lx - h - 2;          // frame pixel of window pixel (0, 0)
        }
    }
    // ---- the window: (V + 5)^2 pixels; off the frame, non-finite or (under the V x V pixels) masked: the star fails
    int bad = live ? 0 : 1;
    if (live) {
        for (int k = tid; k < W * W; k += PSB_BLOCK) {
            const int a = k / W, b = k - a * W;
            const long long y = (long long)y0 + a, x = (long long)x0 + b;
            float v = 0.f;
            if (y < 0 || y >= ny || x < 0 || x >= nx) bad = 1;
            else {
                v = img[(size_t)y * nx + x];
                if (!finite_f32(v)) bad = 1;
                if (mask && a >= 2 && a < V + 2 && b >= 2 && b < V + 2 && mask[(size_t)y * nx + x]) bad = 1;
            }
            s_win[k] = v;
        }
    }
    bad = __syncthreads_or(bad);
    double norm = 0.0;
    if (!bad) {
        float wy[6], wx[6];
        psb_taps(fy, wy); psb_taps(fx, wx);
        double qy = 0.0, qx = 0.0;
#pragma unroll
        for (int j = 0; j < 6; j++) { qy += (double)wy[j] * (double)wy[j]; qx += (double)wx[j] * (double)wx[j]; }
        const double q = qy * qx;
        for (int k = tid; k < W * V; k += PSB_BLOCK) {               // row pass
            const int a = k / V, c = k - a * V;
            const float* p = s_win + a * W + c;
            float t = wx[0] * p[0];
#pragma unroll
            for (int j = 1; j < 6; j++) t += wx[j] * p[j];
            s_row[k] = t;
        }
        __syncthreads();
        double part = 0.0;
        for (int k = tid; k < npx; k += PSB_BLOCK) {                 // column pass
            const int r = k / V, c = k - r * V;
            const float* p = s_row + r * V + c;
            float t = wy[0] * p[0];
#pragma unroll
            for (int j = 1; j < 6; j++) t += wy[j] * p[j * V];
            s_st[k] = t;
            if ((r - h) * (r - h) + (c - h) * (c - h) <= h * h) part += (double)t;
        }
        norm = wg_sum_seq<PSB_BLOCK / 64>(part, s_red);
        if (!(norm > 0.0) || !(norm < 1.0e300)) bad = 1;             // (uniform: every thread holds the same norm)
        if (!bad) {
            const double s2 = (double)sg * (double)sg, n2 = norm * norm;
            for (int k = tid; k < npx; k += PSB_BLOCK) {
                const float t = s_st[k];
                const float I = (float)((double)t / norm);
                const double aI = (double)acc * (double)I;
                const double var = q * ((double)fmaxf(t, 0.f) + s2) / n2 + aI * aI;
                oI[k] = I;
                ow[k] = (float)(1.0 / var);
            }
        }
    }
    if (bad) {
        for (int k = tid; k < npx; k += PSB_BLOCK) { oI[k] = 0.f; ow[k] = 0.f; }
    }
    if (tid == 0) { out_norm[s] = bad ? 0.0 : norm; out_ok[s] = bad ? 0 : 1; }
}

extern "C" int bbx_psf_stamps(bbx_ctx* ctx, int ny, int nx, const float* d_img, const uint8_t* d_mask, int nsrc, const int32_t* d_ys,
                              const int32_t* d_xs, const float* d_shapes, const float* d_sig, int nstar, const int32_t* d_star,
                              const int32_t* d_nstar, int V, float acc, float* d_I, float* d_w, double* d_norm, uint8_t* d_ok,
                              void* stream) {
    if (!ctx || ny < 1 || nx < 1 || nsrc < 0 || nstar < 0 || V < 1 || V > PSB_VMAX || !(V & 1) || !(acc >= 0.f)) return BBX_ERR_ARG;
    if (nstar == 0) return BBX_OK;
    if (!d_img || !d_I || !d_w || !d_norm || !d_ok) return BBX_ERR_ARG;
    if (nsrc > 0 && (!d_ys || !d_xs || !d_shapes || !d_sig)) return BBX_ERR_ARG;
    hipLaunchKernelGGL(k_psf_stamps, dim3(nstar), dim3(PSB_BLOCK), 0, (hipStream_t)stream, ny, nx, d_img, d_mask, nsrc, d_ys, d_xs, d_shapes,
                       d_sig, d_star, d_nstar, V, acc, d_I, d_w, d_norm, d_ok);
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// weighted least squares per vignette pixel
// ---------------------------------------------------------------------------------------------------------------------
template <int NC>
__global__ __launch_bounds__(PSB_FIT_BLOCK) void k_psf_fit(int nstar, int npix, const float* __restrict__ I, const float* __restrict__ w,
                                                           const float* __restrict__ terms, const uint8_t* __restrict__ ok,
                                                           const float* __restrict__ chi2, const float* __restrict__ chi2_med, float clip,
                                                           float* __restrict__ basis, int32_t* __restrict__ d_err) {
    constexpr int NA = NC * (NC + 1) / 2, NT = NA + NC;
    __shared__ double s_acc[NT * 64];                                // 33 KB at NC = 10
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p = blockIdx.x * 64 + lane;
    const bool on = p < npix;
    double A[NA], b[NC];
#pragma unroll
    for (int k = 0; k < NA; k++) A[k] = 0.0;
#pragma unroll
    for (int k = 0; k < NC; k++) b[k] = 0.0;
    const int share = (nstar + PSB_FIT_WAVES - 1) / PSB_FIT_WAVES;
    const int s0 = min(wave * share, nstar), s1 = min(s0 + share, nstar);
    const float gate = chi2 ? clip * chi2_med[0] : 0.f;
    for (int s = s0; s < s1; s++) {                                  // (every condition here is uniform per wave)
        if (!ok[s]) continue;
        if (chi2 && !(chi2[s] <= gate)) continue;
        const float* t = terms + (size_t)s * NC;
        const double ws = on ? (double)w[(size_t)s * npix + p] : 0.0;
        const double Is = on ? (double)I[(size_t)s * npix + p] : 0.0;
        int a = 0;
#pragma unroll
        for (int k = 0; k < NC; k++) {
            const double wt = ws * (double)t[k];
#pragma unroll
            for (int l = 0; l <= k; l++) A[a++] += wt * (double)t[l];
            b[k] += wt * Is;
        }
    }
    // the waves' partial sums, added in wave order
    for (int wv = 0; wv < PSB_FIT_WAVES; wv++) {
        if (wave == wv) {
#pragma unroll
            for (int k = 0; k < NA; k++) s_acc[k * 64 + lane] = wv ? s_acc[k * 64 + lane] + A[k] : A[k];
#pragma unroll
            for (int k = 0; k < NC; k++) s_acc[(NA + k) * 64 + lane] = wv ? s_acc[(NA + k) * 64 + lane] + b[k] : b[k];
        }
        __syncthreads();
    }
    if (wave != 0 || !on) return;
#pragma unroll
    for (int k = 0; k < NA; k++) A[k] = s_acc[k * 64 + lane];
#pragma unroll
    for (int k = 0; k < NC; k++) b[k] = s_acc[(NA + k) * 64 + lane];
    // Cholesky A = L L^T in place (row-packed lower triangle: A[k (k + 1) / 2 + l], l <= k)
    bool pd = true;
#pragma unroll
    for (int k = 0; k < NC; k++) {
#pragma unroll
        for (int l = 0; l <= k; l++) {
            double v = A[k * (k + 1) / 2 + l];
#pragma unroll
            for (int j = 0; j < l; j++) v -= A[k * (k + 1) / 2 + j] * A[l * (l + 1) / 2 + j];
            if (l == k) {
                const double d0 = A[k * (k + 1) / 2 + k];
                if (!(v > PSB_PD_EPS * d0) || !(d0 < 1.0e300)) { pd = false; v = 1.0; }
                A[k * (k + 1) / 2 + k] = sqrt(v);
            } else
                A[k * (k + 1) / 2 + l] = v / A[l * (l + 1) / 2 + l];
        }
    }
#pragma unroll
    for (int k = 0; k < NC; k++) {                                   // L y = b
        double v = b[k];
#pragma unroll
        for (int j = 0; j < k; j++) v -= A[k * (k + 1) / 2 + j] * b[j];
        b[k] = v / A[k * (k + 1) / 2 + k];
    }
#pragma unroll
    for (int k = NC - 1; k >= 0; k--) {                              // L^T a = y
        double v = b[k];
#pragma unroll
        for (int j = k + 1; j < NC; j++) v -= A[j * (j + 1) / 2 + k] * b[j];
        b[k] = v / A[k * (k + 1) / 2 + k];
    }
#pragma unroll
    for (int k = 0; k < NC; k++) basis[(size_t)k * npix + p] = pd ? (float)b[k] : 0.f;
    if (!pd) atomicOr(d_err, BBX_DERR_NOTCONV);
}

extern "C" int bbx_psf_fit(bbx_ctx* ctx, int nstar, int V, int ncoef, const float* d_I, const float* d_w, const float* d_terms,
                           const uint8_t* d_ok, const float* d_chi2, const float* d_chi2_med, float clip, float* d_basis, void* stream) {
    if (!ctx || nstar < 1 || V < 1 || V > PSB_VMAX || !(V & 1) || (ncoef != 1 && ncoef != 3 && ncoef != 6 && ncoef != 10) || !d_I || !d_w ||
        !d_terms || !d_ok || !d_basis || (d_chi2 && (!d_chi2_med || !(clip > 0.f))))
        return BBX_ERR_ARG;
    const int npix = V * V;
    const dim3 grid((npix + 63) / 64), blk(PSB_FIT_BLOCK);
    hipStream_t st = (hipStream_t)stream;
#define PSB_FIT(NC) hipLaunchKernelGGL(k_psf_fit<NC>, grid, blk, 0, st, nstar, npix, d_I, d_w, d_terms, d_ok, d_chi2, d_chi2_med, clip, d_basis, ctx->d_err)
    if (ncoef == 1) PSB_FIT(1);
    else if (ncoef == 3) PSB_FIT(3);
    else if (ncoef == 6) PSB_FIT(6);
    else PSB_FIT(10);
#undef PSB_FIT
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// chi^2 of every star against the model at its position
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PSB_BLOCK) void k_psf_chi2(int npix, int ncoef, const float* __restrict__ I, const float* __restrict__ w,
                                                        const float* __restrict__ terms, const float* __restrict__ basis,
                                                        const uint8_t* __restrict__ ok, float* __restrict__ chi2) {
    __shared__ double s_red[PSB_BLOCK / 64];
    const int s = blockIdx.x, tid = threadIdx.x;
    if (!ok[s]) {                                                    // (uniform per workgroup)
        if (tid == 0) chi2[s] = __builtin_nanf("");
        return;
    }
    float t[PSB_NCOEF_MAX];
#pragma unroll
    for (int k = 0; k < PSB_NCOEF_MAX; k++) t[k] = k < ncoef ? terms[(size_t)s * ncoef + k] : 0.f;
    double part = 0.0;
    for (int p = tid; p < npix; p += PSB_BLOCK) {
        float m = 0.f;
#pragma unroll
        for (int k = 0; k < PSB_NCOEF_MAX; k++)
            if (k < ncoef) m = __builtin_fmaf(t[k], basis[(size_t)k * npix + p], m);
        const double d = (double)I[(size_t)s * npix + p] - (double)m;
        part += (double)w[(size_t)s * npix + p] * (d * d);
    }
    const double tot = wg_sum_seq<PSB_BLOCK / 64>(part, s_red);
    if (tid == 0) chi2[s] = (float)(tot / (double)npix);
}

extern "C" int bbx_psf_chi2(bbx_ctx* ctx, int nstar, int V, int ncoef, const float* d_I, const float* d_w, const float* d_terms,
                            const float* d_basis, const uint8_t* d_ok, float* d_chi2, void* stream) {
    if (!ctx || nstar < 0 || V < 1 || V > PSB_VMAX || !(V & 1) || ncoef < 1 || ncoef > PSB_NCOEF_MAX) return BBX_ERR_ARG;
    if (nstar == 0) return BBX_OK;
    if (!d_I || !d_w || !d_terms || !d_basis || !d_ok || !d_chi2) return BBX_ERR_ARG;
    hipLaunchKernelGGL(k_psf_chi2, dim3(nstar), dim3(PSB_BLOCK), 0, (hipStream_t)stream, V * V, ncoef, d_I, d_w, d_terms, d_basis, d_ok,
                       d_chi2);
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}
