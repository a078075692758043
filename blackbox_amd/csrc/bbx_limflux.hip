// bbx_limflux.hip -- limiting-flux image of the reduced frame (include/bbx.h, bbx_limflux_image): at every pixel
// nsigma / sqrt(sum Q W), the PSF^2-weighted correlation of the inverse-variance image W = 1 / sigma^2 with the squared,
// normalised stamp Q of the pixel's tile, over the central T x T pixels that hold 1 - frac of Q.
//
//   k_lim_window : one workgroup of 256 per tile.  norm (float64), Q = (P / norm)^2 rounded to float32 once, the ring sums of Q in
//                  float64 (ring m = the pixels at Chebyshev distance m from the centre, one thread per ring, row-major), T, and the
//                  table the frame kernel reads: qt[i][p], i < T the window's column, p < 64, = Q[h - k + p - 7][h - k + i] for
//                  0 <= p - 7 < T and 0 elsewhere -- column-major and zero-padded by 7 in front, so that the eight outputs of a lane
//                  take their eight coefficients of one W row from eight consecutive words
//   k_lim_frame  : blocks of 64 x 32 output pixels laid out per tile (partial blocks at tile and frame edges), so that Q and T are
//                  uniform in a workgroup.  W of the block and its halo of k is formed once in LDS (mask, sigma and the frame's edge
//                  applied there).  Lane = column; wave w owns rows 8 w .. 8 w + 7 and holds eight sums in registers.  Per stamp
//                  column i and per W row r one LDS read feeds eight fmaf's, the coefficients qt[i][r .. r + 7] are wave-uniform
//                  (scalar loads).  The W rows are taken four at a time, T + 7 rounded up to a multiple of 4; the rows past the
//                  halo are zero in LDS and meet zero coefficients.  The order of a pixel's sum is i ascending, then j ascending.
//                  Sigma off a mini image: k_spl_polytable (bbx_spline.h) tabulates the cubic of every row and interval first, a
//                  pixel of W then costs a 16-byte load and a Horner step and has bbx_spl_eval's bits
#include "bbx_spline.h"

#define LIM_BLOCK 256
#define LIM_BX    64                                  // output columns of a block: one per lane
#define LIM_R     8                                   // output rows of a lane
#define LIM_BY    (LIM_R * LIM_BLOCK / 64)            // output rows of a block: 32
#define LIM_SMAX  BBX_LIMFLUX_SMAX
#define LIM_QP    64                                  // words of one column of qt: T + 2 * 7 <= 63
#define LIM_WMAX  3.402823466e38f                     // the largest float32: W where sigma * sigma underflows
#define LIM_CH    4                                   // W rows per step of the inner loop
#define LIM_ROWS  (LIM_BY - LIM_R + ((LIM_SMAX + LIM_R - 1 + LIM_CH - 1) / LIM_CH) * LIM_CH)     // 24 + 56 = 80
#define LIM_COLS  (LIM_BX + LIM_SMAX - 1)             // 112
static_assert(LIM_SMAX + 2 * (LIM_R - 1) < LIM_QP, "a zero-padded column of qt fits its 64 words");
static_assert(((LIM_SMAX + LIM_R - 1 + LIM_CH - 1) / LIM_CH) * LIM_CH + LIM_R - 1 <= LIM_QP, "the last step's coefficients lie inside the column");
static_assert(LIM_ROWS * LIM_COLS * 4 <= 64 * 1024, "the W block fits the static LDS limit");

// rows of W a wave walks through for a window of T: T + 7, rounded up to whole steps
__host__ __device__ static inline int lim_nrr(int T) { return ((T + LIM_R - 1 + LIM_CH - 1) / LIM_CH) * LIM_CH; }

__global__ __launch_bounds__(LIM_BLOCK) void k_lim_window(const float* __restrict__ planes, int S, double frac, int32_t* __restrict__ win,
                                                          float* __restrict__ qt, int32_t* __restrict__ d_win) {
    __shared__ float s_q[LIM_SMAX * LIM_SMAX];
    __shared__ double s_red[LIM_BLOCK / 64];
    __shared__ double s_ring[LIM_SMAX / 2 + 1];
    __shared__ int s_T;
    const int tid = threadIdx.x, t = blockIdx.x, npx = S * S, h = S / 2;
    const float* P = planes + (size_t)t * npx;
    for (int p = tid; p < npx; p += LIM_BLOCK) s_q[p] = P[p];
    __syncthreads();
    double part = 0.0;
    for (int p = tid; p < npx; p += LIM_BLOCK) part += (double)s_q[p];
    const double norm = wg_sum_seq<LIM_BLOCK / 64>(part, s_red);
    const bool ok = norm > 0.0 && norm < 1.0e300;                    // positive and finite (a NaN fails both)
    __syncthreads();
    for (int p = tid; p < npx; p += LIM_BLOCK) {
        const double v = (double)s_q[p] / norm;
        s_q[p] = ok ? (float)(v * v) : 0.f;
    }
    __syncthreads();
    if (tid <= h) {                                                  // ring m = tid, row-major
        const int m = tid;
        double r = 0.0;
        if (m == 0) r = (double)s_q[h * S + h];
        else {
            for (int i = -m; i <= m; i++) r += (double)s_q[(h - m) * S + h + i];
            for (int j = -m + 1; j <= m - 1; j++) { r += (double)s_q[(h + j) * S + h - m]; r += (double)s_q[(h + j) * S + h + m]; }
            for (int i = -m; i <= m; i++) r += (double)s_q[(h + m) * S + h + i];
        }
        s_ring[m] = r;
    }
    __syncthreads();
    if (tid == 0) {
        int T = 0;
        if (ok) {
            double tot = 0.0;
            for (int m = 0; m <= h; m++) tot += s_ring[m];
            T = S;
            if (frac != 0.0) {
                const double want = (1.0 - frac) * tot;
                double c = 0.0;
                for (int m = 0; m <= h; m++) {
                    c += s_ring[m];
                    if (c >= want) { T = 2 * m + 1; break; }
                }
            }
        }
        s_T = T;
        win[t] = T;
        if (d_win) d_win[t] = T;
    }
    __syncthreads();
    const int T = s_T, k = T / 2;
    float* q = qt + (size_t)t * LIM_SMAX * LIM_QP;
    for (int e = tid; e < T * LIM_QP; e += LIM_BLOCK) {
        const int i = e / LIM_QP, p = e - i * LIM_QP, jj = p - (LIM_R - 1);
        q[e] = (jj >= 0 && jj < T) ? s_q[(h - k + jj) * S + (h - k + i)] : 0.f;
    }
}

struct lim_args {
    const float* sigma; const uint8_t* mask; const int32_t* win; const float* qt; float* lim;
    int ny, nx, size, nsy, nsx, nbx, nby;
    float nsigma;
};

// block index along one axis -> the tile it lies in, its first pixel and the end of its tile's pixels (exclusive).  Tiles before the
// last have nb blocks each; the last tile takes what is left of the frame
__device__ __forceinline__ void lim_place(int b, int nb, int size, int nt, int n, int blk, int& tile, int& p0, int& pend) {
    tile = min(b / nb, nt - 1);
    p0 = tile * size + (b - tile * nb) * blk;
    pend = tile < nt - 1 ? min((tile + 1) * size, n) : n;
}

// bbx_spl_eval with the cubic of (row, interval) taken from the table k_spl_polytable made of bbx_spl_poly: the same bits, without
// folding sixteen float64 coefficients per pixel
__device__ __forceinline__ float lim_spl_eval(const bbx_spl& sp, int Y, int X) {
    int c, r;
    bbx_spl_axis(X, sp.pw, sp.rpw, sp.px, sp.npad, sp.nx1, sp.dx, sp.rdx, c, r);
    return bbx_spl_horner(sp.poly[(size_t)Y * sp.cnx + c], (float)r * sp.rdx);
}

template <bool MINI>
__global__ __launch_bounds__(LIM_BLOCK) void k_lim_frame(lim_args a, bbx_spl sp) {
    __shared__ float s_w[LIM_ROWS * LIM_COLS];
    int ty, tx, y0, x0, yend, xend;
    lim_place((int)blockIdx.y, a.nby, a.size, a.nsy, a.ny, LIM_BY, ty, y0, yend);
    lim_place((int)blockIdx.x, a.nbx, a.size, a.nsx, a.nx, LIM_BX, tx, x0, xend);
    if (y0 >= yend || x0 >= xend) return;                            // (the whole workgroup: before any barrier)
    const int t = ty * a.nsx + tx;
    const int T = __builtin_amdgcn_readfirstlane(a.win[t]);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int yo = y0 + wave * LIM_R, xo = x0 + lane;                // the lane's first output pixel
    if (T <= 0) {                                                    // a stamp without a sum
        if (xo < xend)
            for (int o = 0; o < LIM_R; o++)
                if (yo + o < yend) a.lim[(size_t)(yo + o) * a.nx + xo] = 0.f;
        return;
    }
    const int k = T / 2, nrr = lim_nrr(T);
    const int pitch = LIM_BX + 2 * k, rows = LIM_BY - LIM_R + nrr, rows_in = LIM_BY + 2 * k;
    // ---- W of the block and its halo; the rows past the halo are zero
    for (int e = tid; e < rows * pitch; e += LIM_BLOCK) {
        const int r = e / pitch, c = e - r * pitch;
        const int y = y0 - k + r, x = x0 - k + c;
        float w = 0.f;
        if (r < rows_in && y >= 0 && y < a.ny && x >= 0 && x < a.nx) {
            const size_t ix = (size_t)y * a.nx + x;
            if (!(a.mask && a.mask[ix])) {
                const float sg = MINI ? lim_spl_eval(sp, y, x) : a.sigma[ix];
                if (finite_f32(sg) && sg > 0.f) w = fminf(1.0f / (sg * sg), LIM_WMAX);     // (finite: the zero coefficients of the padding meet it)
            }
        }
        s_w[e] = w;
    }
    __syncthreads();
    // ---- the sums
    float acc[LIM_R];
#pragma unroll
    for (int o = 0; o < LIM_R; o++) acc[o] = 0.f;
    const float* __restrict__ qt = a.qt + (size_t)t * LIM_SMAX * LIM_QP;
    const float* wl = s_w + wave * LIM_R * pitch + lane;
    for (int i = 0; i < T; i++) {
        const float* __restrict__ qi = qt + i * LIM_QP;
        const float* wc = wl + i;
        for (int r0 = 0; r0 < nrr; r0 += LIM_CH) {
            float q[LIM_CH + LIM_R - 1];
#pragma unroll
            for (int e = 0; e < LIM_CH + LIM_R - 1; e++) q[e] = qi[r0 + e];          // wave-uniform
#pragma unroll
            for (int u = 0; u < LIM_CH; u++) {
                const float w = wc[(r0 + u) * pitch];
#pragma unroll
                for (int o = 0; o < LIM_R; o++) acc[o] = fmaf(q[u + LIM_R - 1 - o], w, acc[o]);
            }
        }
    }
    if (xo < xend) {
#pragma unroll
        for (int o = 0; o < LIM_R; o++)
            if (yo + o < yend) a.lim[(size_t)(yo + o) * a.nx + xo] = acc[o] > 0.f ? a.nsigma / sqrtf(acc[o]) : 0.f;
    }
}

static inline int lim_blocks(int n, int size, int nt, int blk, int* nb) {
    *nb = (size + blk - 1) / blk;
    const long long last = (long long)n - (long long)(nt - 1) * size;
    return (nt - 1) * *nb + (last > 0 ? (int)((last + blk - 1) / blk) : 1);
}

extern "C" int bbx_limflux_image(bbx_ctx* ctx, int ny, int nx, const float* d_sigma, const bbx_spline_image* sigma_mini,
                                 const uint8_t* d_mask, int S, const float* d_planes, int size, int nsy, int nsx, float nsigma, double frac,
                                 float* d_lim, int32_t* d_win, void* stream) {
    if (!ctx || ny < 0 || nx < 0 || size < 1 || nsy < 1 || nsx < 1 || S < 1 || S > LIM_SMAX || !(S & 1)) return BBX_ERR_ARG;
    if (!(frac >= 0.0) || !(frac < 1.0) || !(nsigma > 0.f) || !(nsigma < 3.0e38f)) return BBX_ERR_ARG;
    if ((long long)nsy * nsx > (1 << 20) || (long long)(nsy - 1) * size > 0x7fffffffLL - 2 * LIM_BX ||
        (long long)(nsx - 1) * size > 0x7fffffffLL - 2 * LIM_BX) return BBX_ERR_ARG;
    if ((long long)ny * nx == 0) return BBX_OK;                                             // (an empty frame has no pointers to give)
    if ((d_sigma != nullptr) == (sigma_mini != nullptr)) return BBX_ERR_ARG;                // one form
    if (!d_planes || !d_lim) return BBX_ERR_ARG;
    bbx_spl sp = {};
    if (sigma_mini) {
        const int rc = bbx_spl_make(sigma_mini, ny, nx, &sp);
        if (rc) return rc;
    }
    const int nsub = nsy * nsx;
    const size_t win_bytes = ((size_t)nsub * sizeof(int32_t) + 255) & ~(size_t)255;
    int rc;
    const size_t qt_bytes = (size_t)nsub * LIM_SMAX * LIM_QP * sizeof(float);
    const size_t tab_bytes = sigma_mini ? (size_t)ny * sp.cnx * sizeof(float4) : 0;          // the cubics of every row (bbx_spline.h)
    char* ws = (char*)bbx_ws(ctx, WS_LIMFLUX, win_bytes + qt_bytes + tab_bytes, &rc);
    if (!ws) return rc;
    lim_args a = {};
    a.sigma = d_sigma; a.mask = d_mask; a.win = (const int32_t*)ws; a.qt = (const float*)(ws + win_bytes); a.lim = d_lim;
    a.ny = ny; a.nx = nx; a.size = size; a.nsy = nsy; a.nsx = nsx; a.nsigma = nsigma;
    const int gx = lim_blocks(nx, size, nsx, LIM_BX, &a.nbx), gy = lim_blocks(ny, size, nsy, LIM_BY, &a.nby);
    if (gy > 65535) return BBX_ERR_ARG;
    hipLaunchKernelGGL(k_lim_window, dim3(nsub), dim3(LIM_BLOCK), 0, (hipStream_t)stream, d_planes, S, frac, (int32_t*)ws,
                       (float*)(ws + win_bytes), d_win);
    BBX_LAUNCH_CHECK();
    if (sigma_mini) {
        float4* tab = (float4*)(ws + win_bytes + qt_bytes);
        hipLaunchKernelGGL(k_spl_polytable, dim3((sp.cnx + 255) / 256, ny), dim3(256), 0, (hipStream_t)stream, sp, ny, tab);
        BBX_LAUNCH_CHECK();
        sp.poly = tab;
    }
    if (sigma_mini)
        hipLaunchKernelGGL(k_lim_frame<true>, dim3(gx, gy), dim3(LIM_BLOCK), 0, (hipStream_t)stream, a, sp);
    else
        hipLaunchKernelGGL(k_lim_frame<false>, dim3(gx, gy), dim3(LIM_BLOCK), 0, (hipStream_t)stream, a, sp);
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}
