// bbx_transfit.hip -- transient vetting (include/bbx.h, bbx_zogy_pd_stamps, bbx_trans_psffit and bbx_trans_shapefit):
// the PSF of the difference image D per sub-image, per transient candidate a fit of that PSF to D with free position, and
// per candidate an elliptical Gaussian and an elliptical Moffat fitted to D by Levenberg-Marquardt (at the end of the file).
//
//   bbx_zogy_pd_stamps : P_D^ = (fr fn / fD) Pr^ Pn^ / sqrt(sn^2 fr^2 |Pr^|^2 + sr^2 fn^2 |Pn^|^2) on an M x M grid, back to real
//                        space, cut to S x S.  The stamps have S x S pixels, so the forward transforms are plain matrix DFTs
//                        (S taps per output); everything in float64 (twiddles from sincospi), p is real, so only the columns
//                        kx <= M / 2 are made.
//     k_pd_cols   one workgroup per (kx, sub-image): the two stamps' row sums A[v] = sum_u P[v][u] w^(kx u), the column
//                 Pn^[.][kx], Pr^[.][kx] from them, P_D^[.][kx] into LDS, its inverse along y for all M rows -> C[sub][y][kx]
//     k_pd_rows   one workgroup per (y, sub-image): p[y][x] for all x from C[y][0 .. M / 2]; the pixels of the stamp go to
//                 raw[sub][S][S] (float64), the row's sum of |p| and the part of it inside the stamp to rowsum
//     k_pd_finish one workgroup per sub-image: unit sum in float64, float32 stamp, fold; dead tiles
//   bbx_trans_psffit   : one workgroup of 256 per candidate.  The window's D and V_D are formed once in LDS; every iteration
//                        shifts the sub-image's P_D stamp by theta (psb_shift_stamp: steps 2, 3 of bbx_psf_optflux_shift),
//                        takes the nine sums of the 3 x 3 normal equations in one block reduction and every thread solves them.
//   Sums: per thread over pixels tid, tid + 256, ..., the wave by DPP, the four waves in order: no atomics, same input, same bits.
#include "bbx_spline.h"

#define TF_BLOCK 256
#define TF_SMAX  49
#define TF_WMAX  39                                                  // bbx_trans_psffit: W <= S - 10; bbx_trans_shapefit: W <= TF_WMAX
#define TF_MMAX  512
#define TF_NSUM  9

struct tf_scal { float sn, sr, fn, fr, dx, dy; };

__device__ __forceinline__ bool tf_pos(float v) { return finite_f32(v) && v > 0.f; }
__device__ __forceinline__ bool tf_fin(double v) { return fabs(v) <= 1.0e300; }                                   // (false for NaN)

// ---- P_D ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void tf_twiddles(double2* tw, int M) {
    for (int k = threadIdx.x; k < M; k += TF_BLOCK) {
        double s, c;
        sincospi(2.0 * (double)k / (double)M, &s, &c);
        tw[k] = make_double2(c, s);
    }
}

__global__ __launch_bounds__(TF_BLOCK) void k_pd_cols(const float* __restrict__ pn, const float* __restrict__ pr, const tf_scal* __restrict__ sc,
                                                      int S, int M, double2* __restrict__ C) {
    __shared__ double2 tw[TF_MMAX], col[TF_MMAX], A[2][TF_SMAX];
    const int tid = threadIdx.x, kx = blockIdx.x, sub = blockIdx.y, h = S / 2, MH = M / 2 + 1;
    tf_twiddles(tw, M);
    __syncthreads();
    if (tid < 2 * S) {
        // A[v] = sum_u P[v][u] exp(-2 pi i kx (u - h) / M)
        const int which = tid / S, v = tid - which * S;
        const float* p = (which ? pr : pn) + ((size_t)sub * S + v) * S;
        int e = (int)(((long long)kx * (M - h)) % M);
        double ax = 0.0, ay = 0.0;
        for (int u = 0; u < S; u++) {
            const double q = (double)p[u];
            ax += q * tw[e].x; ay -= q * tw[e].y;
            e += kx; if (e >= M) e -= M;
        }
        A[which][v] = make_double2(ax, ay);
    }
    __syncthreads();
    const tf_scal z = sc[sub];
    const double sn = z.sn, sr = z.sr, fn = z.fn, fr = z.fr;
    const double sn2 = sn * sn, sr2 = sr * sr, fn2 = fn * fn, fr2 = fr * fr;
    const double fD = fr * fn / sqrt(sn2 * fr2 + sr2 * fn2), q = (fr * fn) / fD;
    for (int ky = tid; ky < M; ky += TF_BLOCK) {
        int e = (int)(((long long)ky * (M - h)) % M);
        double nx_ = 0.0, ny_ = 0.0, rx = 0.0, ry = 0.0;
        for (int v = 0; v < S; v++) {
            const double2 t = tw[e], a = A[0][v], b = A[1][v];
            nx_ += a.x * t.x + a.y * t.y; ny_ += a.y * t.x - a.x * t.y;
            rx += b.x * t.x + b.y * t.y; ry += b.y * t.x - b.x * t.y;
            e += ky; if (e >= M) e -= M;
        }
        const double pn2 = nx_ * nx_ + ny_ * ny_, pr2 = rx * rx + ry * ry;
        const double den = (sn2 * fr2) * pr2 + (sr2 * fn2) * pn2;
        double2 o = make_double2(0.0, 0.0);
        if (den > 0.0) {
            const double f = q / sqrt(den);
            o = make_double2((rx * nx_ - ry * ny_) * f, (rx * ny_ + ry * nx_) * f);
        }
        col[ky] = o;
    }
    __syncthreads();
    // C[y][kx] = sum_ky P_D^[ky][kx] exp(+2 pi i ky y / M)
    for (int y = tid; y < M; y += TF_BLOCK) {
        int e = 0;
        double cx = 0.0, cy = 0.0;
        for (int ky = 0; ky < M; ky++) {
            const double2 t = tw[e], a = col[ky];
            cx += a.x * t.x - a.y * t.y; cy += a.x * t.y + a.y * t.x;
            e += y; if (e >= M) e -= M;
        }
        C[((size_t)sub * M + y) * MH + kx] = make_double2(cx, cy);
    }
}

// the stamp index of grid coordinate g (the stamp's centre on the origin, negative offsets wrapped), -1 outside
__device__ __forceinline__ int tf_stamp_index(int g, int M, int h) { return g <= h ? g + h : (g >= M - h ? g - M + h : -1); }

__global__ __launch_bounds__(TF_BLOCK) void k_pd_rows(const double2* __restrict__ C, int S, int M, double* __restrict__ raw, double* __restrict__ rowsum) {
    __shared__ double2 tw[TF_MMAX], c[TF_MMAX / 2 + 1];
    __shared__ double s_red[TF_BLOCK / 64];
    const int tid = threadIdx.x, y = blockIdx.x, sub = blockIdx.y, h = S / 2, MH = M / 2 + 1;
    tf_twiddles(tw, M);
    for (int k = tid; k < MH; k += TF_BLOCK) c[k] = C[((size_t)sub * M + y) * MH + k];
    __syncthreads();
    const int sy = tf_stamp_index(y, M, h);
    const double inv = 1.0 / ((double)M * (double)M);
    double tot = 0.0, in = 0.0;
    for (int x = tid; x < M; x += TF_BLOCK) {
        double acc = 0.0;
        int e = x; if (e >= M) e -= M;
        for (int kx = 1; kx < M / 2; kx++) {
            const double2 t = tw[e], a = c[kx];
            acc += a.x * t.x - a.y * t.y;
            e += x; if (e >= M) e -= M;
        }
        const double p = ((c[0].x + ((x & 1) ? -c[M / 2].x : c[M / 2].x)) + 2.0 * acc) * inv;
        const int sx = tf_stamp_index(x, M, h);
        tot += fabs(p);
        if (sy >= 0 && sx >= 0) {
            in += fabs(p);
            raw[((size_t)sub * S + sy) * S + sx] = p;
        }
    }
    tot = wg_sum_seq<TF_BLOCK / 64>(tot, s_red);
    in = wg_sum_seq<TF_BLOCK / 64>(in, s_red);
    if (tid == 0) {
        rowsum[((size_t)sub * M + y) * 2] = tot;
        rowsum[((size_t)sub * M + y) * 2 + 1] = in;
    }
}

__global__ __launch_bounds__(TF_BLOCK) void k_pd_finish(const float* __restrict__ pn, const float* __restrict__ pr, const tf_scal* __restrict__ sc, int S, int M,
                                                        const double* __restrict__ raw, const double* __restrict__ rowsum, float* __restrict__ pd,
                                                        float* __restrict__ fold) {
    __shared__ double s_red[TF_BLOCK / 64];
    const int tid = threadIdx.x, sub = blockIdx.x, npx = S * S;
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = tid; k < npx; k += TF_BLOCK) {
        v[0] += raw[(size_t)sub * npx + k];
        v[1] += (double)pn[(size_t)sub * npx + k];
        v[2] += (double)pr[(size_t)sub * npx + k];
    }
    for (int y = tid; y < M; y += TF_BLOCK) {
        v[3] += rowsum[((size_t)sub * M + y) * 2];
        v[4] += rowsum[((size_t)sub * M + y) * 2 + 1];
    }
#pragma unroll
    for (int q = 0; q < 5; q++) v[q] = wg_sum_seq<TF_BLOCK / 64>(v[q], s_red);
    const tf_scal z = sc[sub];
    const bool live = tf_pos(z.sn) && tf_pos(z.sr) && tf_pos(z.fn) && tf_pos(z.fr) && v[1] > 0.0 && tf_fin(v[1]) && v[2] > 0.0 && tf_fin(v[2]) &&
                      v[0] > 0.0 && tf_fin(v[0]) && v[3] > 0.0 && tf_fin(v[3]);
    for (int k = tid; k < npx; k += TF_BLOCK) pd[(size_t)sub * npx + k] = live ? (float)(raw[(size_t)sub * npx + k] / v[0]) : 0.f;
    if (tid == 0) fold[sub] = live ? (float)((v[3] - v[4]) / v[3]) : 1.f;
}

static inline size_t tf_up(size_t b) { return (b + 255) & ~(size_t)255; }

extern "C" int bbx_zogy_pd_stamps(bbx_ctx* ctx, int nsub, int S, int M, const float* d_pn, const float* d_pr, const float* h_scal, float* d_pd,
                                  float* d_fold, void* stream) {
    if (!ctx || nsub < 0 || S < 1 || S > TF_SMAX || !(S & 1) || M < 4 * S || M > TF_MMAX || (M & 1)) return BBX_ERR_ARG;
    if (nsub == 0) return BBX_OK;
    if (!d_pn || !d_pr || !h_scal || !d_pd || !d_fold || nsub > 65535) return BBX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int MH = M / 2 + 1;
    const size_t b_sc = tf_up((size_t)nsub * sizeof(tf_scal)), b_C = tf_up((size_t)nsub * M * MH * sizeof(double2)),
                 b_raw = tf_up((size_t)nsub * S * S * sizeof(double)), b_row = tf_up((size_t)nsub * M * 2 * sizeof(double));
    int rc;
    char* w = (char*)bbx_ws(ctx, WS_TRANSFIT, b_sc + b_C + b_raw + b_row, &rc); if (rc) return rc;
    tf_scal* sc = (tf_scal*)w;
    double2* C = (double2*)(w + b_sc);
    double* raw = (double*)(w + b_sc + b_C);
    double* rowsum = (double*)(w + b_sc + b_C + b_raw);
    BBX_HIP(hipMemcpyAsync(sc, h_scal, (size_t)nsub * sizeof(tf_scal), hipMemcpyHostToDevice, s));               // pageable source: staged before the call returns
    hipLaunchKernelGGL(k_pd_cols, dim3(MH, nsub), dim3(TF_BLOCK), 0, s, d_pn, d_pr, sc, S, M, C);
    hipLaunchKernelGGL(k_pd_rows, dim3(M, nsub), dim3(TF_BLOCK), 0, s, C, S, M, raw, rowsum);
    hipLaunchKernelGGL(k_pd_finish, dim3(nsub), dim3(TF_BLOCK), 0, s, d_pn, d_pr, sc, S, M, raw, rowsum, d_pd, d_fold);
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}

// ---- the fit ----------------------------------------------------------------------------------------------------------------
// what the window of a candidate is read from: the frames, the two sigma maps as frames (the mini images travel beside it), the
// mask, the sub-images' scalars and their grid
struct tf_win {
    const float *D, *N, *R, *sig_n, *sig_r; const uint8_t* mask; const tf_scal* sc;
    int ny, nx, size, nsx, nsy;
};
struct tf_args {
    tf_win w; const float* pd;
    const int32_t *ys, *xs;
    float *flux, *err, *dy, *dx, *chi2; uint8_t* flags;
    int S, W, niter; float maxshift;
};

__device__ __forceinline__ int tf_sub_index(const tf_win& w, int py, int px) {
    return min(max(py, 0) / w.size, w.nsy - 1) * w.nsx + min(max(px, 0) / w.size, w.nsx - 1);
}

// The window of W x W pixels around the peak (py, px), pixels first, first + stride, ... : D into s_d, V_D = (fr^2 Vn + fn^2 Vr) /
// (fr fn)^2 in float32 into s_v (0: the pixel is not used -- off the frame, masked, D not finite, V_D not positive and finite;
// s_d is 0 there).  hit: a masked pixel was left out; the return value counts the used pixels of this thread.  The one place
// where the used-pixel rule and V_D are written down: bbx_trans_psffit and bbx_trans_shapefit both fit on this window
template <bool MINI>
__device__ __forceinline__ double tf_window(const tf_win& w, const bbx_spl& spn, const bbx_spl& spr, const tf_scal& z, int py, int px, bool nofit, int W,
                                            int first, int stride, float* s_d, float* s_v, int& hit) {
    const int nw = W * W, hw = W / 2;
    const float fr2 = z.fr * z.fr, fn2 = z.fn * z.fn, ff = z.fr * z.fn, ff2 = ff * ff;
    double cnt = 0.0;
    for (int k = first; k < nw; k += stride) {
        const int wy = k / W, wx = k - wy * W;
        const long long y = (long long)py - hw + wy, x = (long long)px - hw + wx;
        float d = 0.f, v = 0.f;
        if (!nofit && y >= 0 && y < w.ny && x >= 0 && x < w.nx) {
            const size_t ix = (size_t)y * w.nx + (size_t)x;
            if (w.mask && w.mask[ix]) hit = 1;
            else {
                d = w.D[ix];
                if (finite_f32(d)) {
                    const float sn = MINI ? bbx_spl_eval(spn, (int)y, (int)x) : w.sig_n[ix];
                    const float sr = MINI ? bbx_spl_eval(spr, (int)y, (int)x) : w.sig_r[ix];
                    const float vn = fmaxf(w.N[ix], 0.f) + sn * sn, vr = fmaxf(w.R[ix], 0.f) + sr * sr;
                    v = (fr2 * vn + fn2 * vr) / ff2;
                    if (!(v > 0.f) || !finite_f32(v)) v = 0.f;
                }
                if (v == 0.f) d = 0.f;
            }
        }
        s_d[k] = d; s_v[k] = v;
        if (v > 0.f) cnt += 1.0;
    }
    return cnt;
}

template <bool MINI>
__global__ __launch_bounds__(TF_BLOCK) void k_trans_psffit(tf_args a, bbx_spl spn, bbx_spl spr) {
    __shared__ float s_a[TF_SMAX * TF_SMAX];                         // 9.6 KB each: the stamp, and the row pass's output
    __shared__ float s_b[TF_SMAX * TF_SMAX];
    __shared__ float s_d[TF_WMAX * TF_WMAX], s_v[TF_WMAX * TF_WMAX]; // 6.1 KB each: D and V_D of the window (V_D = 0: pixel not used)
    __shared__ double s_red[TF_BLOCK / 64 * TF_NSUM];
    __shared__ double s_red1[TF_BLOCK / 64];
    const int tid = threadIdx.x, c = blockIdx.x;
    const int S = a.S, npx = S * S, h = S / 2, W = a.W, nw = W * W, hw = W / 2;
    const int py = a.ys[c], px = a.xs[c];
    unsigned fl = 0;
    bool nofit = py < 0 || py >= a.w.ny || px < 0 || px >= a.w.nx;   // (uniform, like everything that steers the flow below)
    const int sub = tf_sub_index(a.w, py, px);
    const tf_scal z = a.w.sc[sub];
    const float* pd = a.pd + (size_t)sub * npx;
    // ---- the window: D and V_D in float32
    int hit = 0;
    double cnt[1];
    cnt[0] = tf_window<MINI>(a.w, spn, spr, z, py, px, nofit, W, tid, TF_BLOCK, s_d, s_v, hit);
    if (__syncthreads_or(hit)) fl |= 2u;
    wg_sum_seq<TF_BLOCK / 64>(cnt, s_red);
    const int n_used = (int)cnt[0];
    if (n_used < 4) nofit = true;

    // the stamp of the sub-image moved to theta and its unit-sum norm; false: the stamp has no sum
    auto place = [&](float ty, float tx, double& norm) -> bool {
        __syncthreads();                                             // (s_a may still be read from the pass before)
        for (int k = tid; k < npx; k += TF_BLOCK) s_a[k] = pd[k];
        __syncthreads();
        psb_shift_stamp<TF_BLOCK>(s_a, s_b, S, ty, tx);
        norm = psb_stamp_sum<TF_BLOCK>(s_a, npx, s_red1);
        return norm > 0.0 && norm < 1.0e300;
    };
    const int w0 = (h - hw) * S + (h - hw);                          // stamp index of the window's first pixel
    float ty = 0.f, tx = 0.f;
    bool stopped = false;
    double last = 0.0;
    const double bound = (double)a.maxshift;
    for (int it = 0; it < a.niter && !nofit && !stopped; it++) {
        double norm;
        if (!place(ty, tx, norm)) { nofit = true; break; }
        // normal equations of D ~ F Ps - a Gx - b Gy: u = (Ps, -Gx, -Gy); m00 m01 m02 m11 m12 m22, r0 r1 r2
        double q[TF_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int k = tid; k < nw; k += TF_BLOCK) {
            const float vf = s_v[k];
            if (!(vf > 0.f)) continue;
            const int wy = k / W, wx = k - wy * W, i = w0 + wy * S + wx;
            const double v = (double)vf, d = (double)s_d[k];
            const double p = (double)s_a[i] / norm;
            const double ux = -(((double)s_a[i + 1] / norm - (double)s_a[i - 1] / norm) / 2.0);
            const double uy = -(((double)s_a[i + S] / norm - (double)s_a[i - S] / norm) / 2.0);
            q[0] += p * p / v; q[1] += p * ux / v; q[2] += p * uy / v;
            q[3] += ux * ux / v; q[4] += ux * uy / v; q[5] += uy * uy / v;
            q[6] += p * d / v; q[7] += ux * d / v; q[8] += uy * d / v;
        }
        wg_sum_seq<TF_BLOCK / 64>(q, s_red);
        const double m00 = q[0], m01 = q[1], m02 = q[2], m11 = q[3], m12 = q[4], m22 = q[5], r0 = q[6], r1 = q[7], r2 = q[8];
        const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
        const double det = (m00 * c00 + m01 * c01) + m02 * c02;
        if (!(det != 0.0) || !tf_fin(det)) { stopped = true; break; }
        const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
        const double F = ((c00 * r0 + c01 * r1) + c02 * r2) / det;
        const double ca = ((c01 * r0 + c11 * r1) + c12 * r2) / det;
        const double cb = ((c02 * r0 + c12 * r1) + c22 * r2) / det;
        if (!(F != 0.0) || !tf_fin(F)) { stopped = true; break; }
        const double ddy = cb / F, ddx = ca / F;
        if (!tf_fin(ddy) || !tf_fin(ddx)) { stopped = true; break; }
        last = fmax(fabs(ddy), fabs(ddx));
        const double sy = fmin(fmax(ddy, -0.5), 0.5), sx = fmin(fmax(ddx, -0.5), 0.5);
        ty = (float)fmin(fmax((double)ty + sy, -bound), bound);
        tx = (float)fmin(fmax((double)tx + sx, -bound), bound);
    }
    // ---- the final pass at theta
    double F = 0.0, err = 0.0, chi2 = 0.0;
    if (!nofit) {
        double norm;
        if (!place(ty, tx, norm)) nofit = true;
        else {
            double q[2] = {0.0, 0.0};
            for (int k = tid; k < nw; k += TF_BLOCK) {
                const float vf = s_v[k];
                if (!(vf > 0.f)) continue;
                const int wy = k / W, wx = k - wy * W, i = w0 + wy * S + wx;
                const double v = (double)vf, p = (double)s_a[i] / norm;
                q[0] += p * (double)s_d[k] / v; q[1] += p * p / v;
            }
            wg_sum_seq<TF_BLOCK / 64>(q, s_red);
            if (!(q[1] > 0.0) || !tf_fin(q[1]) || !tf_fin(q[0])) nofit = true;
            else {
                F = q[0] / q[1]; err = 1.0 / sqrt(q[1]);
                double r[1] = {0.0};
                for (int k = tid; k < nw; k += TF_BLOCK) {
                    const float vf = s_v[k];
                    if (!(vf > 0.f)) continue;
                    const int wy = k / W, wx = k - wy * W, i = w0 + wy * S + wx;
                    const double e = (double)s_d[k] - F * ((double)s_a[i] / norm);
                    r[0] += e * e / (double)vf;
                }
                wg_sum_seq<TF_BLOCK / 64>(r, s_red);
                chi2 = r[0] / (double)(n_used - 3);
            }
        }
    }
    if (tid == 0) {
        if (nofit) {
            fl = (fl & 2u) | 4u;
            a.flux[c] = a.err[c] = a.dy[c] = a.dx[c] = a.chi2[c] = 0.f;
        } else {
            if (fabsf(ty) >= a.maxshift || fabsf(tx) >= a.maxshift) fl |= 1u;
            if (stopped || last > 0.01) fl |= 8u;
            a.flux[c] = (float)F; a.err[c] = (float)err; a.dy[c] = ty; a.dx[c] = tx; a.chi2[c] = (float)chi2;
        }
        a.flags[c] = (uint8_t)fl;
    }
}

extern "C" int bbx_trans_psffit(bbx_ctx* ctx, int ny, int nx, const float* d_D, const float* d_N, const float* d_R, const float* d_sig_n,
                                const float* d_sig_r, const bbx_spline_image* mini_n, const bbx_spline_image* mini_r, const uint8_t* d_mask, int S,
                                int nsub, const float* d_pd, int size, int nsx, const float* h_scal, int ncand, const int32_t* d_ys,
                                const int32_t* d_xs, int W, int niter, float maxshift, float* d_flux, float* d_err, float* d_dy, float* d_dx,
                                float* d_chi2, uint8_t* d_flags, void* stream) {
    if (!ctx || ny < 1 || nx < 1 || S < 1 || S > TF_SMAX || !(S & 1) || W < 3 || !(W & 1) || W > S - 10 || ncand < 0) return BBX_ERR_ARG;
    if (size < 1 || nsx < 1 || nsub < nsx || nsub % nsx || nsub > 65535 || niter < 1 || niter > 64) return BBX_ERR_ARG;
    if (!(maxshift > 0.f) || !(maxshift <= 16.f)) return BBX_ERR_ARG;
    const bool mini = mini_n != nullptr || mini_r != nullptr;
    if (mini ? (!mini_n || !mini_r || d_sig_n || d_sig_r) : (!d_sig_n || !d_sig_r)) return BBX_ERR_ARG;               // one form, for both
    bbx_spl spn = {}, spr = {};
    if (mini) {
        int rc = bbx_spl_make(mini_n, ny, nx, &spn); if (rc) return rc;
        rc = bbx_spl_make(mini_r, ny, nx, &spr); if (rc) return rc;
    }
    if (!d_D || !d_N || !d_R || !d_pd || !h_scal) return BBX_ERR_ARG;
    if (ncand == 0) return BBX_OK;
    if (!d_ys || !d_xs || !d_flux || !d_err || !d_dy || !d_dx || !d_chi2 || !d_flags) return BBX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    int rc;
    tf_scal* sc = (tf_scal*)bbx_ws(ctx, WS_TRANSFIT, tf_up((size_t)nsub * sizeof(tf_scal)), &rc); if (rc) return rc;
    BBX_HIP(hipMemcpyAsync(sc, h_scal, (size_t)nsub * sizeof(tf_scal), hipMemcpyHostToDevice, s));               // pageable source: staged before the call returns
    const tf_args a = {{d_D, d_N, d_R, d_sig_n, d_sig_r, d_mask, sc, ny, nx, size, nsx, nsub / nsx}, d_pd, d_ys, d_xs,
                       d_flux, d_err, d_dy, d_dx, d_chi2, d_flags, S, W, niter, maxshift};
    if (mini)
        hipLaunchKernelGGL(k_trans_psffit<true>, dim3(ncand), dim3(TF_BLOCK), 0, s, a, spn, spr);
    else
        hipLaunchKernelGGL(k_trans_psffit<false>, dim3(ncand), dim3(TF_BLOCK), 0, s, a, spn, spr);
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}

// ---- the shape fits: an elliptical Gaussian and an elliptical Moffat fitted to D per candidate (bbx_trans_shapefit) ----
// One wave per candidate, TS_WAVES candidates per workgroup.  Every lane keeps the pixels lane, lane + 64, ... of its wave's
// window; the 36 sums of a pass go per lane over those pixels, then over the wave by DPP (wave_sum_f64: the result in every
// lane), so the reductions need no workgroup barrier and every lane runs the same small float64 algebra on the same numbers.
#define TS_WAVES 4
#define TS_NPAR  7                                                   // A, B, y0, x0, cyy, cxy, cxx
#define TS_NH    28
#define TS_NSUM  36                                                  // H (upper triangle by rows), g, chi2
#define TS_NMIN  8

struct ts_args {
    tf_win w; const float* fwhm0; const int32_t *ys, *xs; float* out; uint8_t* flags;
    int ncand, W, niter, models; float maxshift, beta, lo, hi;
};

__device__ __forceinline__ constexpr int ts_h(int i, int j) { return i * TS_NPAR - i * (i - 1) / 2 + (j - i); }       // i <= j
__device__ __forceinline__ constexpr int ts_l(int i, int j) { return i * (i + 1) / 2 + j; }                           // j <= i

// the sums at p over the wave's window: H = sum J J^T / V, g = sum J r / V, chi2 = sum r^2 / V; m = B + A g(q),
// q = cyy dy^2 + 2 cxy dy dx + cxx dx^2 about (y0, x0), g = exp(-q / 2) or (1 + q)^-beta
__device__ __forceinline__ void ts_pass(bool moffat, double beta, const double (&p)[TS_NPAR], const float* s_d, const float* s_v, int W, int lane,
                                        double (&s)[TS_NSUM]) {
    const int nw = W * W, hw = W / 2;
#pragma unroll
    for (int q = 0; q < TS_NSUM; q++) s[q] = 0.0;
    for (int k = lane; k < nw; k += 64) {
        const float vf = s_v[k];
        if (!(vf > 0.f)) continue;
        const int wy = k / W, wx = k - wy * W;
        const double v = (double)vf, d = (double)s_d[k];
        const double dy = (double)(wy - hw) - p[2], dx = (double)(wx - hw) - p[3];
        const double q = p[4] * dy * dy + 2.0 * p[5] * dy * dx + p[6] * dx * dx;
        double g, gq;
        if (moffat) { g = pow(1.0 + q, -beta); gq = -beta * g / (1.0 + q); }
        else { g = exp(-0.5 * q); gq = -0.5 * g; }
        const double a = p[0] * gq;
        const double J[TS_NPAR] = {g, 1.0, a * (-2.0 * (p[4] * dy + p[5] * dx)), a * (-2.0 * (p[5] * dy + p[6] * dx)), a * (dy * dy), a * (2.0 * dy * dx),
                                   a * (dx * dx)};
        const double r = d - (p[1] + p[0] * g);
        double Jw[TS_NPAR];
#pragma unroll
        for (int i = 0; i < TS_NPAR; i++) Jw[i] = J[i] / v;
#pragma unroll
        for (int i = 0; i < TS_NPAR; i++) {
#pragma unroll
            for (int j = i; j < TS_NPAR; j++) s[ts_h(i, j)] += J[i] * Jw[j];
            s[TS_NH + i] += Jw[i] * r;
        }
        s[TS_NSUM - 1] += r * r / v;
    }
#pragma unroll
    for (int q = 0; q < TS_NSUM; q++) s[q] = wave_sum_f64(s[q]);
}

// L of H + lam diag H (lower triangle by rows); false at a pivot that is not positive and finite.  hold2, hold3: y0, x0 are held --
// their rows and columns count 0 off the diagonal
__device__ __forceinline__ bool ts_chol(const double (&H)[TS_NSUM], double lam, double (&L)[TS_NH], bool hold2 = false, bool hold3 = false) {
#pragma unroll
    for (int j = 0; j < TS_NPAR; j++) {
        double s = H[ts_h(j, j)] * (1.0 + lam);
#pragma unroll
        for (int k = 0; k < j; k++) s -= L[ts_l(j, k)] * L[ts_l(j, k)];
        if (!(s > 0.0 && s <= 1.0e300)) return false;
        L[ts_l(j, j)] = sqrt(s);
#pragma unroll
        for (int i = j + 1; i < TS_NPAR; i++) {
            double t = H[ts_h(j, i)];
            if ((hold2 && (i == 2 || j == 2)) || (hold3 && (i == 3 || j == 3))) t = 0.0;
#pragma unroll
            for (int k = 0; k < j; k++) t -= L[ts_l(i, k)] * L[ts_l(j, k)];
            L[ts_l(i, j)] = t / L[ts_l(j, j)];
        }
    }
    return true;
}

__device__ __forceinline__ void ts_solve(const double (&L)[TS_NH], const double* b, double (&x)[TS_NPAR]) {
#pragma unroll
    for (int i = 0; i < TS_NPAR; i++) {
        double t = b[i];
#pragma unroll
        for (int k = 0; k < i; k++) t -= L[ts_l(i, k)] * x[k];
        x[i] = t / L[ts_l(i, i)];
    }
#pragma unroll
    for (int i = TS_NPAR - 1; i >= 0; i--) {
        double t = x[i];
#pragma unroll
        for (int k = i + 1; k < TS_NPAR; k++) t -= L[ts_l(k, i)] * x[k];
        x[i] = t / L[ts_l(i, i)];
    }
}

// sqrt diag (L L^T)^-1: M = L^-1 column by column, diag_i = sum_{k >= i} M[k][i]^2
__device__ __forceinline__ void ts_errors(const double (&L)[TS_NH], double (&e)[TS_NPAR]) {
#pragma unroll
    for (int i = 0; i < TS_NPAR; i++) {
        double col[TS_NPAR];
        col[i] = 1.0 / L[ts_l(i, i)];
        double s = col[i] * col[i];
#pragma unroll
        for (int k = i + 1; k < TS_NPAR; k++) {
            double t = 0.0;
#pragma unroll
            for (int j = i; j < k; j++) t -= L[ts_l(k, j)] * col[j];
            col[k] = t / L[ts_l(k, k)];
            s += col[k] * col[k];
        }
        e[i] = sqrt(s);
    }
}

// the axes of the form: FWHM = 2 sqrt(kk / l) of the eigenvalues l1 >= l2; false: not finite or not positive definite
__device__ __forceinline__ bool ts_axes(double kk, double cyy, double cxy, double cxx, double& fmin_, double& fmaj, double& l1, double& l2) {
    if (!tf_fin(cyy) || !tf_fin(cxy) || !tf_fin(cxx) || !(cyy > 0.0 && cxx > 0.0 && cyy * cxx - cxy * cxy > 0.0)) return false;
    const double hd = 0.5 * (cyy - cxx), root = sqrt(hd * hd + cxy * cxy), mean = 0.5 * (cyy + cxx);
    l1 = mean + root;
    l2 = (cyy * cxx - cxy * cxy) / l1;                               // (not mean - root: no cancellation)
    if (!(l2 > 0.0 && tf_fin(l1))) return false;
    fmin_ = 2.0 * sqrt(kk / l1); fmaj = 2.0 * sqrt(kk / l2);
    return true;
}

template <bool MINI>
__global__ __launch_bounds__(TS_WAVES * 64) void k_trans_shapefit(ts_args a, bbx_spl spn, bbx_spl spr) {
    __shared__ float s_dd[TS_WAVES][TF_WMAX * TF_WMAX], s_vv[TS_WAVES][TF_WMAX * TF_WMAX];       // 48.7 KB
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c = blockIdx.x * TS_WAVES + wv;
    const bool live = c < a.ncand;                                   // (uniform over the wave, like everything that steers the flow below)
    float* s_d = s_dd[wv];
    float* s_v = s_vv[wv];
    const int W = a.W, nw = W * W, hw = W / 2;
    const int py = live ? a.ys[c] : -1, px = live ? a.xs[c] : -1;
    bool nofit = py < 0 || py >= a.w.ny || px < 0 || px >= a.w.nx;
    const int sub = tf_sub_index(a.w, py, px);
    const tf_scal z = a.w.sc[sub];
    int hit = 0;
    const double cnt = tf_window<MINI>(a.w, spn, spr, z, py, px, nofit, W, lane, 64, s_d, s_v, hit);
    __syncthreads();                                                 // the one barrier: the start below reads other lanes' pixels
    if (!live) return;
    unsigned fl = __builtin_amdgcn_ballot_w64(hit != 0) ? 2u : 0u;
    const int n_used = (int)wave_sum_f64(cnt);
    const double lo = (double)a.lo, hi = (double)a.hi, bound = (double)a.maxshift, beta = (double)a.beta;
    double f0 = (double)a.fwhm0[sub];
    if (n_used < TS_NMIN || !(f0 > 0.0) || !tf_fin(f0)) nofit = true;
    f0 = fmin(fmax(f0, lo), hi);
    // A starts at D of the peak pixel, or of the used pixel of largest |D| (the first of those in row-major order)
    double A0 = 0.0;
    if (!nofit) {
        const int kp = hw * W + hw;
        if (s_v[kp] > 0.f) A0 = (double)s_d[kp];
        else {
            float best = -1.f;
            for (int k = 0; k < nw; k++)
                if (s_v[k] > 0.f && fabsf(s_d[k]) > best) { best = fabsf(s_d[k]); A0 = (double)s_d[k]; }
        }
    }
    for (int mi = 0; mi < 2; mi++) {
        const bool moffat = mi == 1;
        float res[TS_NPAR] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        unsigned f = (fl & 2u) | 4u;
        if (!nofit && (a.models & (1 << mi))) {
            const double kk = moffat ? exp2(1.0 / beta) - 1.0 : 2.0 * 0.69314718055994530942;
            const double c0 = 4.0 * kk / (f0 * f0);
            double p[TS_NPAR] = {A0, 0.0, 0.0, 0.0, c0, 0.0, c0}, t[TS_NPAR], dl[TS_NPAR], e[TS_NPAR];
            double S[TS_NSUM], St[TS_NSUM], L[TS_NH];
            ts_pass(moffat, beta, p, s_d, s_v, W, lane, S);
            double lam = 1.0e-3;
            bool accepted = false, conv = false, shape_last = false;
            for (int it = 0; it < a.niter; it++) {
                shape_last = false;
                bool ok = false;
                // a centre coordinate at its bound that the gradient pushes further out is held for this step
                const bool hold2 = fabs(p[2]) >= bound && S[TS_NH + 2] * p[2] > 0.0, hold3 = fabs(p[3]) >= bound && S[TS_NH + 3] * p[3] > 0.0;
                if (ts_chol(S, lam, L, hold2, hold3)) {
                    double gs[TS_NPAR];
#pragma unroll
                    for (int i = 0; i < TS_NPAR; i++) gs[i] = S[TS_NH + i];
                    if (hold2) gs[2] = 0.0;
                    if (hold3) gs[3] = 0.0;
                    ts_solve(L, gs, dl);
                    bool finite = true;
#pragma unroll
                    for (int i = 0; i < TS_NPAR; i++) { t[i] = p[i] + dl[i]; finite = finite && tf_fin(t[i]); }
                    double fa, fb, l1, l2;
                    if (!finite || !ts_axes(kk, t[4], t[5], t[6], fa, fb, l1, l2) || !(fa >= lo && fb <= hi)) shape_last = true;
                    else {
                        t[2] = fmin(fmax(t[2], -bound), bound); t[3] = fmin(fmax(t[3], -bound), bound);
                        ts_pass(moffat, beta, t, s_d, s_v, W, lane, St);
                        ok = tf_fin(St[TS_NSUM - 1]) && St[TS_NSUM - 1] <= S[TS_NSUM - 1];
                    }
                }
                if (ok) {
                    // the step against the errors of the undamped H at the point it leaves
                    conv = false;
                    if (ts_chol(S, 0.0, L)) {
                        ts_errors(L, e);
                        conv = true;
#pragma unroll
                        for (int i = 0; i < TS_NPAR; i++) conv = conv && fabs(t[i] - p[i]) <= 0.01 * e[i];
                    }
                    accepted = true;
#pragma unroll
                    for (int i = 0; i < TS_NPAR; i++) p[i] = t[i];
#pragma unroll
                    for (int q = 0; q < TS_NSUM; q++) S[q] = St[q];
                    lam = fmax(lam / 10.0, 1.0e-9);
                } else lam = fmin(lam * 10.0, 1.0e9);
            }
            double fa, fb, l1, l2;
            if (ts_chol(S, 0.0, L) && ts_axes(kk, p[4], p[5], p[6], fa, fb, l1, l2)) {
                ts_errors(L, e);
                const double r[TS_NPAR] = {p[2], p[3], e[2], e[3], sqrt(fa * fb), sqrt(l1 / l2), S[TS_NSUM - 1] / (double)(n_used - TS_NPAR)};
                bool finite = true;
#pragma unroll
                for (int i = 0; i < TS_NPAR; i++) finite = finite && tf_fin(r[i]);
                if (finite) {
#pragma unroll
                    for (int i = 0; i < TS_NPAR; i++) res[i] = (float)r[i];
                    f = fl & 2u;
                    if (fabs(p[2]) >= bound || fabs(p[3]) >= bound) f |= 1u;
                    if (!accepted || !conv) f |= 8u;
                    if (shape_last) f |= 16u;
                }
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < TS_NPAR; i++) a.out[((size_t)mi * TS_NPAR + i) * a.ncand + c] = res[i];
            a.flags[(size_t)mi * a.ncand + c] = (uint8_t)f;
        }
    }
}

extern "C" int bbx_trans_shapefit(bbx_ctx* ctx, int ny, int nx, const float* d_D, const float* d_N, const float* d_R, const float* d_sig_n,
                                  const float* d_sig_r, const bbx_spline_image* mini_n, const bbx_spline_image* mini_r, const uint8_t* d_mask,
                                  int nsub, int size, int nsx, const float* h_scal, const float* d_fwhm0, int ncand, const int32_t* d_ys,
                                  const int32_t* d_xs, int W, int niter, float maxshift, int models, float beta, float fwhm_lo, float fwhm_hi,
                                  float* d_out, uint8_t* d_flags, void* stream) {
    if (!ctx || ny < 1 || nx < 1 || W < 5 || !(W & 1) || W > TF_WMAX || ncand < 0 || ncand > (1 << 28)) return BBX_ERR_ARG;
    if (size < 1 || nsx < 1 || nsub < nsx || nsub % nsx || nsub > 65535 || niter < 1 || niter > 128) return BBX_ERR_ARG;
    if (!(maxshift > 0.f) || !(maxshift <= 16.f) || models < 0 || models > 3 || !(beta > 1.f) || !(beta <= 100.f)) return BBX_ERR_ARG;
    if (!(fwhm_lo > 0.f) || !(fwhm_lo < fwhm_hi) || !(fwhm_hi <= 1.0e6f)) return BBX_ERR_ARG;
    const bool mini = mini_n != nullptr || mini_r != nullptr;
    if (mini ? (!mini_n || !mini_r || d_sig_n || d_sig_r) : (!d_sig_n || !d_sig_r)) return BBX_ERR_ARG;               // one form, for both
    bbx_spl spn = {}, spr = {};
    if (mini) {
        int rc = bbx_spl_make(mini_n, ny, nx, &spn); if (rc) return rc;
        rc = bbx_spl_make(mini_r, ny, nx, &spr); if (rc) return rc;
    }
    if (!d_D || !d_N || !d_R || !h_scal || !d_fwhm0) return BBX_ERR_ARG;
    if (ncand == 0 || models == 0) return BBX_OK;
    if (!d_ys || !d_xs || !d_out || !d_flags) return BBX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    int rc;
    tf_scal* sc = (tf_scal*)bbx_ws(ctx, WS_TRANSSHAPE, tf_up((size_t)nsub * sizeof(tf_scal)), &rc); if (rc) return rc;
    BBX_HIP(hipMemcpyAsync(sc, h_scal, (size_t)nsub * sizeof(tf_scal), hipMemcpyHostToDevice, s));               // pageable source: staged before the call returns
    const ts_args a = {{d_D, d_N, d_R, d_sig_n, d_sig_r, d_mask, sc, ny, nx, size, nsx, nsub / nsx}, d_fwhm0, d_ys, d_xs, d_out, d_flags,
                       ncand, W, niter, models, maxshift, beta, fwhm_lo, fwhm_hi};
    const int nblk = (ncand + TS_WAVES - 1) / TS_WAVES;
    if (mini)
        hipLaunchKernelGGL(k_trans_shapefit<true>, dim3(nblk), dim3(TS_WAVES * 64), 0, s, a, spn, spr);
    else
        hipLaunchKernelGGL(k_trans_shapefit<false>, dim3(nblk), dim3(TS_WAVES * 64), 0, s, a, spn, spr);
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}
