// bbx_objmask.hip -- object mask of a background-subtracted frame: the pixels of the 3x3-smoothed
// frame above nsigma x the box's sigma, their 8-connected components of at least minarea pixels, grown by a disk.
//
// The listed pixels are a few per cent of the frame, so everything behind the detection pass works on the pixel list: the
// union-find of bbx_mask.hip (bbx_cc_count_list) labels it, the sizes are summed per root, and every listed pixel of a
// component that stays stamps its disk into the mask.  The dense passes are the detection read, the mask's clear and the
// count of set pixels.
#include "bbx_common.h"
#include <math.h>

int bbx_cc_count_list(bbx_ctx* ctx, const uint32_t* d_list, const int32_t* d_cnt, size_t cap, int ny, int nx,
                      int32_t* d_out, hipStream_t s);

#define OM_TX 64
#define OM_TY 16
#define OM_GROW_MAX 8

// a tile's (OM_TY + 2) x (OM_TX + 2) pixels, OM_NLOAD per thread: pixel k = tid + 256 j of the tile in row-major order, the
// frame's edge replicated by clamping (so every address is inside the frame, also for the k behind the tile's last pixel)
#define OM_NLOAD (((OM_TY + 2) * (OM_TX + 2) + 255) / 256)
__device__ __forceinline__ void om_tile_fetch(const float* __restrict__ img, int ny, int nx, int ntx, int t, int tid, float (&pre)[OM_NLOAD]) {
    const int ty = t / ntx, tx = t - ty * ntx;
    const int y0 = ty * OM_TY, x0 = tx * OM_TX;
#pragma unroll
    for (int j = 0; j < OM_NLOAD; j++) {
        const int k = tid + 256 * j;
        const int r = k / (OM_TX + 2), c = k - r * (OM_TX + 2);
        const int sy = min(max(y0 - 1 + r, 0), ny - 1), sx = min(max(x0 - 1 + c, 0), nx - 1);
        pre[j] = img[(size_t)sy * nx + sx];
    }
}

// Detection: a workgroup takes tiles of OM_TY x OM_TX pixels with a 1-pixel halo (replicated at the frame's edge) through LDS,
// forms SExtractor's default.conv pyramid -- (((nw+ne)+(sw+se)) + 2((n+s)+(w+e)) + 4c) / 16 in float32, in that order -- and
// lists the pixels with filt >= (float)nsigma * sigma[box] (a sigma that is NaN or <= 0 lists nothing; neither does a NaN or an
// infinity under the 3x3).  Hits go through a per-workgroup LDS queue that is flushed with one global reservation per ~1024
// entries, as in k_compact_abs.
__global__ __launch_bounds__(256) void k_om_detect(const float* __restrict__ img, int ny, int nx, const float* __restrict__ sig, int box,
                                                   int nbx, float nsig, int filter, int ntx, int ntiles, uint32_t* list, int32_t* cnt,
                                                   uint32_t cap, int32_t* err) {
    __shared__ float tile[OM_TY + 2][OM_TX + 2];
    __shared__ uint32_t q[2048];
    __shared__ unsigned qn, gbase;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) qn = 0;
    __syncthreads();
    // the next tile's pixels are fetched into registers while this one is worked on: a workgroup's tiles come one after the
    // other, and without the prefetch each waits out its own loads (0.34 ms for a 10560^2 frame then; bbx_object_mask as a whole
    // 0.52 ms without it, 0.39 ms with it)
    float pre[OM_NLOAD];
    om_tile_fetch(img, ny, nx, ntx, blockIdx.x, tid, pre);                   // (grid <= ntiles)
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {                   // workgroup-uniform
        const int ty = t / ntx, tx = t - ty * ntx;
        const int y0 = ty * OM_TY, x0 = tx * OM_TX;
#pragma unroll
        for (int j = 0; j < OM_NLOAD; j++) {
            const int k = tid + 256 * j;
            if (k < (OM_TY + 2) * (OM_TX + 2)) (&tile[0][0])[k] = pre[j];
        }
        __syncthreads();
        if (t + (int)gridDim.x < ntiles) om_tile_fetch(img, ny, nx, ntx, t + (int)gridDim.x, tid, pre);
        const int x = x0 + lane;
        const int bx = min(x, nx - 1) / box;                                 // the lane's box column; the rows' box row by counting
        int by = (y0 + wv * (OM_TY / 4)) / box, yr = (y0 + wv * (OM_TY / 4)) - by * box;
#pragma unroll
        for (int r = 0; r < OM_TY / 4; r++, yr++) {
            const int ly = wv * (OM_TY / 4) + r, y = y0 + ly;
            if (yr == box) { yr = 0; by++; }
            bool hit = false;
            if (x < nx && y < ny) {
                float f = tile[ly + 1][lane + 1];
                if (filter) {
                    const float corners = (tile[ly][lane] + tile[ly][lane + 2]) + (tile[ly + 2][lane] + tile[ly + 2][lane + 2]);
                    const float sides = (tile[ly][lane + 1] + tile[ly + 2][lane + 1]) + (tile[ly + 1][lane] + tile[ly + 1][lane + 2]);
                    f = ((corners + 2.f * sides) + 4.f * f) * 0.0625f;
                }
                const float thr = nsig * sig[by * nbx + bx];
                hit = thr > 0.f && f >= thr && f < INFINITY;                // NaN compares false
            }
            const unsigned long long m = __builtin_amdgcn_ballot_w64(hit);
            if (m) {
                unsigned wb = 0;
                if (lane == 0) wb = atomicAdd(&qn, (unsigned)__popcll(m));
                wb = __shfl(wb, 0, 64);
                if (hit) q[wb + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))] = (uint32_t)y * (uint32_t)nx + (uint32_t)x;
            }
        }
        __syncthreads();
        const unsigned n = qn;                                               // < 1024 before the tile, <= 1024 from it
        if (n >= 1024 || t + (int)gridDim.x >= ntiles) {
            if (n) {
                if (tid == 0) gbase = atomicAdd((unsigned*)cnt, n);
                __syncthreads();
                const unsigned g0 = gbase;
                for (unsigned k = tid; k < n; k += 256) {
                    if (g0 + k < cap) list[g0 + k] = q[k]; else atomicOr(err, BBX_DERR_LIST_OVERFLOW);
                }
            }
            __syncthreads();
            if (tid == 0) qn = 0;
            __syncthreads();
        }
    }
}

// listed pixels per root (its root: k_cc_flatten ran after the unions)
__global__ __launch_bounds__(256) void k_om_sizes(const int32_t* __restrict__ cnt, int cap, const uint32_t* __restrict__ parent, uint32_t* size) {
    const int n = (*cnt > cap) ? cap : *cnt;
    const int step = (int)(gridDim.x * blockDim.x), nround = (n + step - 1) / step;
    for (int r = 0; r < nround; r++) {
        const int i = r * step + (int)(blockIdx.x * blockDim.x + threadIdx.x);
        const bool on = i < n;
        wave_add_per_root(on, on ? parent[i] : 0u, size);
    }
}

// every listed pixel of a component of at least [minarea] pixels stamps its disk dy^2 + dx^2 <= grow^2, clipped at the frame, with
// plain byte stores of 1 (idempotent: overlapping stamps need no atomics); counts[0] = pixels listed, counts[1] = components kept
__global__ __launch_bounds__(256) void k_om_stamp(const uint32_t* __restrict__ list, const int32_t* __restrict__ cnt, int cap,
                                                  const uint32_t* __restrict__ parent, const uint32_t* __restrict__ size, uint32_t minarea,
                                                  int grow, int ny, int nx, uint8_t* __restrict__ mask, int32_t* counts) {
    const int n = (*cnt > cap) ? cap : *cnt;
    const uint32_t npix = (uint32_t)ny * (uint32_t)nx;
    const int g2 = grow * grow;
    const int step = (int)(gridDim.x * blockDim.x), nround = (n + step - 1) / step;
    int kept = 0;
    for (int r = 0; r < nround; r++) {
        const int i = r * step + (int)(blockIdx.x * blockDim.x + threadIdx.x);
        if (i >= n) continue;
        const uint32_t root = parent[i], p = list[i];
        if (size[root] < minarea || p >= npix) continue;
        kept += (root == (uint32_t)i) ? 1 : 0;
        const int Y = (int)(p / (uint32_t)nx), X = (int)(p - (uint32_t)Y * (uint32_t)nx);
        for (int dy = -grow; dy <= grow; dy++) {
            const int yy = Y + dy;
            if (yy < 0 || yy >= ny) continue;
            int hw = grow;
            while (hw * hw + dy * dy > g2) hw--;                             // >= 0: dy^2 <= grow^2
            const int xa = max(X - hw, 0), xb = min(X + hw, nx - 1);
            uint8_t* row = mask + (size_t)yy * nx;
            for (int xx = xa; xx <= xb; xx++) row[xx] = 1;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[0] = *cnt;
    __shared__ int s_c[4];
    kept = wave_sum_i32(kept);
    if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = kept;
    __syncthreads();
    if (threadIdx.x == 0) { const int t = (s_c[0] + s_c[1]) + (s_c[2] + s_c[3]); if (t) atomicAdd(&counts[1], t); }
}

// pixels set in the mask: 16 bytes per thread and load where the mask is 16-byte aligned, one add per workgroup
__global__ __launch_bounds__(256) void k_om_count(const uint8_t* __restrict__ mask, size_t npix, int32_t* out) {
    const size_t n16 = (((uintptr_t)mask) & 15) ? 0 : npix / 16;
    const uint4* m16 = (const uint4*)mask;
    const size_t stride = (size_t)gridDim.x * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    int c = 0;
    for (size_t i = t0; i < n16; i += stride) {
        const uint4 w = m16[i];
        c += (__popc(w.x & 0x01010101u) + __popc(w.y & 0x01010101u)) + (__popc(w.z & 0x01010101u) + __popc(w.w & 0x01010101u));
    }
    for (size_t i = n16 * 16 + t0; i < npix; i += stride) c += mask[i] & 1;
    __shared__ int s_c[4];
    c = wave_sum_i32(c);
    if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) { const int t = (s_c[0] + s_c[1]) + (s_c[2] + s_c[3]); if (t) atomicAdd(out, t); }
}

extern "C" int bbx_object_mask(bbx_ctx* ctx, int ny, int nx, const float* d_img, const float* d_sig_mini, int box, double nsigma,
                               int minarea, int grow, int filter, int64_t max_pixels, uint8_t* d_objmask, int32_t* d_counts,
                               void* stream) {
    if (!ctx || !d_img || !d_sig_mini || !d_objmask || !d_counts || ny < 1 || nx < 1 || box < 1 || ny % box || nx % box) return BBX_ERR_ARG;
    if (minarea < 1 || grow < 0 || grow > OM_GROW_MAX || !(nsigma > 0.0)) return BBX_ERR_ARG;
    const size_t npix = (size_t)ny * nx;
    if (npix >= ((size_t)1 << 31)) return BBX_ERR_ARG;                       // the counters are int32
    hipStream_t s = (hipStream_t)stream;
    int rc;
    // the list's own capacity: 1/8 of the frame (bbx_cand_cap's 1/16 is too small for a 1.5 sigma isophote), a small frame whole
    size_t cap = max_pixels > 0 ? (size_t)max_pixels : (npix / 8 > (npix < 65536 ? npix : 65536) ? npix / 8 : (npix < 65536 ? npix : 65536));
    if (cap > npix) cap = npix;
    if (cap > ((size_t)1 << 30)) cap = (size_t)1 << 30;                      // list positions + a grid's stride stay inside int32
    uint32_t* list = (uint32_t*)bbx_ws(ctx, WS_CCLIST, cap * sizeof(uint32_t), &rc); if (rc) return rc;
    uint32_t* size = (uint32_t*)bbx_ws(ctx, WS_STAGE2, cap * sizeof(uint32_t), &rc); if (rc) return rc;
    int32_t* cnt = &ctx->d_counters[CNT_CC_N];
    BBX_HIP(hipMemsetAsync(cnt, 0, sizeof(int32_t), s));
    BBX_HIP(hipMemsetAsync(d_counts, 0, 3 * sizeof(int32_t), s));
    BBX_HIP(hipMemsetAsync(d_objmask, 0, npix, s));
    BBX_HIP(hipMemsetAsync(size, 0, cap * sizeof(uint32_t), s));
    const int ntx = (nx + OM_TX - 1) / OM_TX, nty = (ny + OM_TY - 1) / OM_TY;
    const int ntiles = ntx * nty;                                            // < 2^31 / 1024
    hipLaunchKernelGGL(k_om_detect, dim3(ntiles < 2048 ? ntiles : 2048), dim3(256), 0, s, d_img, ny, nx, d_sig_mini, box, nx / box,
                       (float)nsigma, filter ? 1 : 0, ntx, ntiles, list, cnt, (uint32_t)cap, ctx->d_err);
    BBX_LAUNCH_CHECK();
    ctx->cc_roots = 1;                                                       // every pixel's root is read below
    rc = bbx_cc_count_list(ctx, list, cnt, cap, ny, nx, &ctx->d_counters[CNT_CC_ROOTS], s); if (rc) return rc;
    const uint32_t* parent = (const uint32_t*)ctx->d_ws[WS_PARENT];
    hipLaunchKernelGGL(k_om_sizes, dim3(1024), dim3(256), 0, s, cnt, (int)cap, parent, size);
    hipLaunchKernelGGL(k_om_stamp, dim3(1024), dim3(256), 0, s, list, cnt, (int)cap, parent, size, (uint32_t)minarea, grow, ny, nx,
                       d_objmask, d_counts);
    hipLaunchKernelGGL(k_om_count, dim3(1024), dim3(256), 0, s, d_objmask, npix, &d_counts[2]);
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}
