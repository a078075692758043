// bbx_thumb.hip -- transient thumbnails (qc.py:480-485, blackbox.py:2674-2826): the four cut-outs per candidate
// (THUMBNAIL_RED / _REF / _D / _SCORR), the mask flags under the peak, and the 8-bit display planes of the PNG files
// (save_thumbs_row: flipud -> ZScaleInterval().get_limits -> scale_data).
//
//   k_thumb_gather : one workgroup per (candidate, plane); a stream kernel (row-coalesced loads, non-temporal stores)
//   k_thumb_png8   : one workgroup per stamp; the stamp and the 1024-slot sample buffer stay in LDS
#include "bbx_common.h"

#define THUMB_BLOCK   256
#define THUMB_NSAMP   1000          // ZScaleInterval(nsamples=1000)
#define THUMB_SORT    1024          // sort slots: the samples padded with +inf
#define THUMB_LDS_MAX 65536         // what a workgroup gets without opt-in

// ---------------------------------------------------------------------------------------------------------------------
// cut-outs + flags
// ---------------------------------------------------------------------------------------------------------------------
struct thumb_planes { const float* p[4]; };

__global__ __launch_bounds__(THUMB_BLOCK) void k_thumb_gather(int ny, int nx, thumb_planes img, int n, const int32_t* __restrict__ ys,
                                                              const int32_t* __restrict__ xs, int size, const uint8_t* __restrict__ new_mask,
                                                              const uint8_t* __restrict__ ref_mask, int flag_win, float* __restrict__ out,
                                                              uint8_t* __restrict__ flags) {
    const int k = blockIdx.x, plane = blockIdx.y;
    const long long yc = ys[k], xc = xs[k];
    const long long y0 = yc - size / 2, x0 = xc - size / 2;
    const float* __restrict__ src = img.p[plane];
    float* __restrict__ dst = out + ((size_t)k * 4 + plane) * (size_t)size * size;
    const int npx = size * size;
    // consecutive threads -> consecutive columns of a row: 4 * size contiguous bytes per row of the frame
    for (int i = threadIdx.x; i < npx; i += THUMB_BLOCK) {
        const int r = i / size, c = i - r * size;
        const long long y = y0 + r, x = x0 + c;
        float v = 0.f;                                               // off the frame: 0 (this project's convention)
        if (y >= 0 && y < ny && x >= 0 && x < nx) v = src[(size_t)y * nx + x];
        __builtin_nontemporal_store(v, dst + i);
    }
    if (plane != 0 || !flags) return;                                // (uniform per workgroup)
    // FLAGS_MASK: OR of the mask(s) over the flag_win x flag_win window centred on the peak
    __shared__ unsigned s_or;
    if (threadIdx.x == 0) s_or = 0u;
    __syncthreads();
    unsigned m = 0u;
    const long long fy0 = yc - flag_win / 2, fx0 = xc - flag_win / 2;
    for (int i = threadIdx.x; i < flag_win * flag_win; i += THUMB_BLOCK) {
        const int r = i / flag_win, c = i - r * flag_win;
        const long long y = fy0 + r, x = fx0 + c;
        if (y >= 0 && y < ny && x >= 0 && x < nx) {
            m |= new_mask[(size_t)y * nx + x];
            if (ref_mask) m |= ref_mask[(size_t)y * nx + x];
        }
    }
    if (m) atomicOr(&s_or, m);
    __syncthreads();
    if (threadIdx.x == 0) flags[k] = (uint8_t)s_or;
}

extern "C" int bbx_thumbnails(bbx_ctx* ctx, int ny, int nx, const float* const* d_img, int n, const int32_t* d_ys, const int32_t* d_xs,
                              int size, const uint8_t* d_new_mask, const uint8_t* d_ref_mask, int flag_win, float* d_out,
                              uint8_t* d_flags, void* stream) {
    if (!ctx || ny < 1 || nx < 1 || n < 0 || size < 1 || size > 4096 || !d_img) return BBX_ERR_ARG;
    if (n == 0) return BBX_OK;
    if (!d_ys || !d_xs || !d_out || !d_img[0] || !d_img[1] || !d_img[2] || !d_img[3]) return BBX_ERR_ARG;
    if (d_flags && (!d_new_mask || flag_win < 1 || flag_win > 255)) return BBX_ERR_ARG;
    thumb_planes pl;
    for (int i = 0; i < 4; i++) pl.p[i] = d_img[i];
    hipLaunchKernelGGL(k_thumb_gather, dim3(n, 4), dim3(THUMB_BLOCK), 0, (hipStream_t)stream, ny, nx, pl, n, d_ys, d_xs, size,
                       d_new_mask, d_ref_mask, flag_win, d_out, d_flags);
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// display planes: flipud, zscale limits (float64), scale_data (float32, three separately rounded operations)
// ---------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ void thumb_cswap(float& a, float& b, bool up) {
    const float lo = fminf(a, b), hi = fmaxf(a, b);                  // (the samples are finite or +inf: no NaN here)
    a = up ? lo : hi;
    b = up ? hi : lo;
}

__global__ __launch_bounds__(THUMB_BLOCK) void k_thumb_png8(int size, const float* __restrict__ stamps, uint8_t* __restrict__ out_u8,
                                                            double* __restrict__ limits) {
    extern __shared__ __attribute__((aligned(16))) float s_px[];                                 // [size * size]: the flipped stamp
    __shared__ __attribute__((aligned(16))) float s_samp[THUMB_SORT];
    __shared__ uint8_t s_bad[THUMB_SORT];
    __shared__ double s_red[2 * 3 * 4];                              // wg_sum_tree's, up to three sums at once
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int npx = size * size;
    const float* __restrict__ src = stamps + (size_t)blockIdx.x * npx;
    uint8_t* __restrict__ dst = out_u8 + (size_t)blockIdx.x * npx;

    // ---- np.flipud: row r of the display plane is row size-1-r of the cut-out
    for (int i = tid; i < npx; i += THUMB_BLOCK) {
        const int r = i / size, c = i - r * size;
        s_px[(size - 1 - r) * size + c] = __builtin_nontemporal_load(src + i);
    }
    for (int i = tid; i < THUMB_SORT; i += THUMB_BLOCK) s_samp[i] = __builtin_inff();
    __syncthreads();

    // ---- values[np.isfinite(values)][::stride][:1000], in numpy's (C) order: each wave walks a contiguous quarter of the
    // plane 64 pixels at a time; the rank of a finite pixel is the wave's offset + the finite pixels before it
    const int seg = ((npx + 3) / 4 + 63) / 64 * 64;
    const int beg = wave * seg, end = min(npx, beg + seg);
    int run = 0;
    for (int b = beg; b < end; b += 64) {
        const int i = b + lane;
        const bool fin = i < end && finite_f32(s_px[i]);
        run += __popcll(__ballot(fin));
    }
    if (lane == 0) s_cnt[wave] = run;
    __syncthreads();
    const int c0 = s_cnt[0], c1 = s_cnt[1], c2 = s_cnt[2], c3 = s_cnt[3];
    const int count = c0 + c1 + c2 + c3;
    const int stride = max(1, count / THUMB_NSAMP);                  // int(max(1.0, size / nsamples))
    const int npix = min(THUMB_NSAMP, (count + stride - 1) / stride);
    run = wave == 0 ? 0 : wave == 1 ? c0 : wave == 2 ? c0 + c1 : c0 + c1 + c2;
    for (int b = beg; b < end; b += 64) {
        const int i = b + lane;
        const float v = i < end ? s_px[i] : __builtin_nanf("");
        const bool fin = finite_f32(v);
        const unsigned long long mask = __ballot(fin);
        const int rank = run + __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
        if (fin) {
            const int q = rank / stride;
            if (q * stride == rank && q < THUMB_NSAMP) s_samp[q] = v;
        }
        run += __popcll(mask);
    }
    __syncthreads();

    // ---- samples.sort(): bitonic network over the 1024 slots.  The steps with partner distance >= 4 go through LDS, two
    // compare-exchanges per thread (distances >= 32 are conflict-free on the 32 banks of a half-wave, 4..16 two-way); the last
    // two steps of every phase (distances 2 and 1) are done on four consecutive slots in registers (one ds_read_b128).
    for (int kk = 2; kk <= THUMB_SORT; kk <<= 1) {
        for (int j = kk >> 1; j >= 4; j >>= 1) {
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int t = tid + h * THUMB_BLOCK;
                const int i = 2 * j * (t / j) + (t % j);
                float a = s_samp[i], b = s_samp[i + j];
                thumb_cswap(a, b, (i & kk) == 0);
                s_samp[i] = a; s_samp[i + j] = b;
            }
            __syncthreads();
        }
        float4 q = ((float4*)s_samp)[tid];
        const int i0 = 4 * tid;
        if (kk >= 4) {
            const bool up = (i0 & kk) == 0;
            thumb_cswap(q.x, q.z, up); thumb_cswap(q.y, q.w, up);
            thumb_cswap(q.x, q.y, up); thumb_cswap(q.z, q.w, up);
        } else {                                                     // kk == 2: pairs (0,1) up, (2,3) down
            thumb_cswap(q.x, q.y, true); thumb_cswap(q.z, q.w, false);
        }
        ((float4*)s_samp)[tid] = q;
        __syncthreads();
    }

    // ---- the iterative line fit on the sorted samples (float64; weights 0/1; the weighted least-squares line in closed form)
    double vmin = 0.0, vmax = 0.0;
    if (npix > 0) {
        const float smin = s_samp[0], smax = s_samp[npix - 1];
        vmin = (double)smin; vmax = (double)smax;
        const int minpix = max(5, npix / 2);                         // max(min_npixels, int(npix * max_reject))
        const int ngrow = max(1, (int)((double)npix * 0.01));         // max(1, int(npix * 0.01))
        const int gs = (ngrow - 1) / 2;                              // numpy.convolve(..., 'same'): out[i] = OR in[i + gs - ngrow + 1 .. i + gs]
        double y[4]; bool ok[4], bad[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int x = tid + j * THUMB_BLOCK;
            ok[j] = x < npix; bad[j] = false;
            y[j] = ok[j] ? (double)s_samp[x] : 0.0;
        }
        int ngood = npix, last = npix + 1, ph = 0;
        double slope = 0.0;
        for (int it = 0; it < 5; it++) {                             // (every quantity below is the same in all threads)
            if (ngood >= last || ngood < minpix) break;
            double a[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (ok[j] && !bad[j]) { a[0] += 1.0; a[1] += (double)(tid + j * THUMB_BLOCK); a[2] += y[j]; }
            wg_sum_tree<THUMB_BLOCK / 64>(a, s_red, ph);
            const double nw = a[0], xm = a[1] / nw, ym = a[2] / nw;
            double b[2] = {0.0, 0.0};
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (ok[j] && !bad[j]) { const double dx = (double)(tid + j * THUMB_BLOCK) - xm; b[0] += dx * dx; b[1] += dx * (y[j] - ym); }
            wg_sum_tree<THUMB_BLOCK / 64>(b, s_red, ph);
            slope = b[1] / b[0];
            const double icpt = ym - slope * xm;
            double flat[4], c[1] = {0.0};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                flat[j] = y[j] - (slope * (double)(tid + j * THUMB_BLOCK) + icpt);
                if (ok[j] && !bad[j]) c[0] += flat[j];
            }
            wg_sum_tree<THUMB_BLOCK / 64>(c, s_red, ph);
            const double mf = c[0] / nw;
            double d[1] = {0.0};
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (ok[j] && !bad[j]) { const double e = flat[j] - mf; d[0] += e * e; }
            wg_sum_tree<THUMB_BLOCK / 64>(d, s_red, ph);
            const double thr = 2.5 * sqrt(d[0] / nw);                // krej * flat[~badpix].std()
#pragma unroll
            for (int j = 0; j < 4; j++)
                s_bad[tid + j * THUMB_BLOCK] = (bad[j] || flat[j] < -thr || flat[j] > thr) ? 1 : 0;
            __syncthreads();
            double g[1] = {0.0};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int x = tid + j * THUMB_BLOCK;
                bool bb = false;
                if (ok[j]) {
                    const int lo = max(0, x + gs - ngrow + 1), hi = min(npix - 1, x + gs);
                    for (int u = lo; u <= hi; u++) bb = bb || s_bad[u];
                    if (!bb) g[0] += 1.0;
                }
                bad[j] = bb;
            }
            wg_sum_tree<THUMB_BLOCK / 64>(g, s_red, ph);             // (its barrier also ends the reads of s_bad)
            last = ngood;
            ngood = (int)g[0];
        }
        if (ngood >= minpix) {
            slope = slope / 0.25;                                    // contrast
            const int cpix = (npix - 1) / 2;
            // np.median of the float32 samples: float32 mean of the middle pair
            const float med = (npix & 1) ? s_samp[npix / 2] : __fdiv_rn(__fadd_rn(s_samp[npix / 2 - 1], s_samp[npix / 2]), 2.0f);
            vmin = fmax(vmin, (double)med - (double)(cpix - 1) * slope);
            vmax = fmin(vmax, (double)med + (double)(npix - cpix) * slope);
        }
    }
    if (tid == 0 && limits) { limits[2 * (size_t)blockIdx.x] = vmin; limits[2 * (size_t)blockIdx.x + 1] = vmax; }

    // ---- scale_data: data -= vmin; data /= (vmax - vmin); data *= 255 in float32, clip, astype('uint8') (NaN -> 0)
    const float f_min = (float)vmin, f_rng = (float)(vmax - vmin);
    const bool flat_stamp = !(npix > 0) || vmax == vmin;             // our convention: all zeros
    auto scale = [&](float v) -> unsigned {
        if (flat_stamp) return 0u;
        float t = __fmul_rn(__fdiv_rn(__fsub_rn(v, f_min), f_rng), 255.0f);
        if (!(t > 0.f)) return 0u;                                   // < 0 and NaN
        if (t > 255.f) t = 255.f;
        return (unsigned)t;
    };
    if ((npx & 3) == 0) {
        uint32_t* __restrict__ dst4 = (uint32_t*)dst;                // (npx % 4 == 0: every stamp starts on a 4-byte boundary)
        for (int i = tid; i < npx / 4; i += THUMB_BLOCK) {
            const float4 q = ((const float4*)s_px)[i];
            const uint32_t w = scale(q.x) | (scale(q.y) << 8) | (scale(q.z) << 16) | (scale(q.w) << 24);
            __builtin_nontemporal_store(w, dst4 + i);
        }
    } else {
        for (int i = tid; i < npx; i += THUMB_BLOCK) dst[i] = (uint8_t)scale(s_px[i]);
    }
}

extern "C" int bbx_thumb_png8(bbx_ctx* ctx, int n_stamps, int size, const float* d_stamps, uint8_t* d_out_u8, double* d_limits,
                              void* stream) {
    if (!ctx || n_stamps < 0 || size < 1) return BBX_ERR_ARG;
    // the stamp + the static arrays of the kernel (sample buffer, flags, reduction scratch) must fit the workgroup's LDS
    const size_t fixed = THUMB_SORT * 4 + THUMB_SORT + 2 * 3 * 4 * 8 + 4 * 4 + 64;
    if ((size_t)size * size * 4 + fixed > THUMB_LDS_MAX) return BBX_ERR_ARG;
    if (n_stamps == 0) return BBX_OK;
    if (!d_stamps || !d_out_u8) return BBX_ERR_ARG;
    if (((size_t)d_out_u8 & 3) != 0) return BBX_ERR_ARG;
    hipLaunchKernelGGL(k_thumb_png8, dim3(n_stamps), dim3(THUMB_BLOCK), (size_t)size * size * 4, (hipStream_t)stream, size, d_stamps,
                       d_out_u8, d_limits);
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}
