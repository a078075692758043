// bbx_common.h -- internal helpers shared by the HIP translation units (gfx950).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/bbx.h"

#define BBX_WAVE 64

struct bbx_dims {
    int ny_raw, nx_raw, ysz, xsz;   // raw shape, channel data section
    int dy, dx;                     // channel size incl. overscans
    int os_y, os_x;                 // overscan rows / columns per channel
    int vos_x0, vos_w;              // vertical overscan strip: column offset in channel, width
    int hos_rows;                   // rows of os_sec_hori (os_y - 10)
    int ny, nx;                     // reduced frame shape
};

// reference define_sections, blackbox.py:6334-6402 (xbin = ybin = 1)
static inline int bbx_make_dims(const bbx_geom* g, bbx_dims* d) {
    if (!g || g->ny_raw <= 0 || g->nx_raw <= 0 || g->ysize_chan <= 0 || g->xsize_chan <= 0)
        return BBX_ERR_ARG;
    d->ny_raw = g->ny_raw; d->nx_raw = g->nx_raw;
    d->ysz = g->ysize_chan; d->xsz = g->xsize_chan;
    if (d->ny_raw % 2 || d->nx_raw % 8) return BBX_ERR_ARG;
    d->dy = d->ny_raw / 2; d->dx = d->nx_raw / 8;
    d->os_y = (d->ny_raw - 2 * d->ysz) / 2;
    d->os_x = (d->nx_raw - 8 * d->xsz) / 8;
    if (d->os_y != d->dy - d->ysz || d->os_x != d->dx - d->xsz) return BBX_ERR_ARG;
    d->hos_rows = d->os_y - 10;            // ncut_hori = 10
    d->vos_x0 = d->xsz + 5;                // ncut_vert = 5
    d->vos_w = d->dx - 1 - d->vos_x0;      // last column dropped
    if (d->hos_rows <= 0 || d->vos_w <= 0) return BBX_ERR_ARG;
    d->ny = 2 * d->ysz; d->nx = 8 * d->xsz;
    return BBX_OK;
}

// device-side error flags (bits) kept in ctx->d_err[0]
#define BBX_DERR_LIST_OVERFLOW 1
#define BBX_DERR_NOTCONV       2
#define BBX_DERR_PSF_WINDOW    4    // bbx_zogy_frame: the PSFs' matched-filter kernels do not fit their row window

// prepared reference data of bbx_zogy_frame (bbx_zogy_refrows, bbx_zogy_refpsf): the caller's buffer (NULL: none) and what it was
// made of -- two inputs by address, the stamp side S (rows: 0) and the geometry (ny, nx, size, border)
struct bbx_zprep { const float2* buf; const void* id[2]; int S; int geom[4]; };

#define BBX_WS_SLOTS 32              // room for the workspace slots of the enum below (WS_MAX; checked there)

struct bbx_ctx {
    int device;
    char hip_err[256];
    // --- persistent small device state
    int32_t* d_err;            // [4] error flags
    // --- work lists (device).  Capacities in elements.
    uint32_t* d_satlist;  int64_t cap_satlist;   // saturated pixel indices (reduced frame)
    void*     flags_clean_ptr; // LA-Cosmic flag plane known to be all-zero (see bbx_lacosmic)
    size_t    flags_clean_bytes;
    void*     d_nonlin;        // nonlin_tab (bbx_calibrate.hip) or NULL
    int       nonlin_on;
    void*     hash_clean_ptr;  // connected-component key table known to be all-empty (see bbx_cc_count_list)
    size_t    hash_clean_n;
    int32_t*  d_counters;      // [CNT_MAX] device counters (see enum below)
    // --- scratch, (re)allocated on demand by bbx_ws()
    void*  d_ws[BBX_WS_SLOTS];
    size_t ws_bytes[BBX_WS_SLOTS];
    int    lac_feed;           // BBX_OPT_LAC_LEVEL_FEED (bbx_set_option)
    int    debug_listcap;      // BBX_OPT_DEBUG_LISTCAP: capacity the LA-Cosmic kernels see (0 = the allocated one)
    void*  zogy_state;         // per-context FFT plans / work buffer of bbx_zogy.hip (NULL until first use)
    void*  zogy_frame_state;   // twiddle table and chunk plan of bbx_zogy_frame (bbx_zogy3.hip)
    int    zogy_kwin_off;      // BBX_OPT_ZOGY_KWIN_OFF: full-size transforms of the matched-filter kernels (no row window)
    int    zogy_ksmall_off;    // BBX_OPT_ZOGY_KSMALL_OFF: k_n, k_r through the full grid even where a small grid exists
    int    sat_attr_set;       // dynamic-LDS attribute of k_trail_segment set through this context
    int    mini_attr_set;      // the same of k_mini_fill_filter_lds
    float  zcand_thr;          // bbx_zogy_candidates: > 0: bbx_zogy_frame lists the pixels with |Scorr| >= thr (WS_ZCAND, CNT_ZCAND)
    const float* zcand_img;    // the Scorr frame the list in WS_ZCAND belongs to (NULL: none); consumed by bbx_find_peaks
    float  zcand_thr_used; size_t zcand_npix;
    bbx_zprep zrows;           // bbx_zogy_refrows: the reference's row transforms; id: the reference frame, its sigma frame or spline coefficients
    bbx_zprep zpsf;            // bbx_zogy_refpsf: the reference PSF's spectra; id: the reference's stamps [nsub][S][S], NULL
    const float* bcand_med;    // bbx_zoom_candidates: device scalar m; the next bbx_spline_zoom_sub lists |out| >= (float)(m * bcand_nsig) (WS_BCAND, CNT_BCAND)
    double bcand_nsig;
    const float* bcand_img;    // the frame the list in WS_BCAND belongs to (consumed by bbx_find_peaks), its median scalar and factor
    const float* bcand_img_med; double bcand_img_nsig; size_t bcand_npix;
    int    wait_sleep_us;      // BBX_OPT_WAIT_SLEEP_US: host waits poll an event and sleep this long between polls (0: hipStreamSynchronize)
    int    cc_roots;           // set by a caller of bbx_cc_count_list that reads the roots afterwards (second k_cc_flatten); cleared by the call
    int    box_pp;             // which of the two CNT_BOXFAIL counters the next bbx_bkg_boxstats call fills
    int    bkg_full_sort;      // BBX_OPT_BKG_FULL_SORT: every box of bbx_bkg_boxstats through the full sort (tests: same statistics as the bracket path)
    int    fpack_hist_only;    // BBX_OPT_FPACK_HIST_ONLY: row medians by radix histograms over all keys (tests: same bytes as the bracket path)
    struct { void* stream; void* ptr; size_t bytes; } fphint[16];   // bbx_fpack_tiles: its row-hint table, one per calling stream (bbx_fpack.hip)
    int    fpack_one_wg;       // BBX_OPT_FPACK_ONE_WG: k_fp_tile with the worst-case stream buffer only (tests: both paths make the same bytes)
    int    spf_attr_bytes;     // dynamic-LDS attribute of the spline prefilter kernels set through this context
    int    zogy3_attr_L;       // sub-image side whose kernels have their dynamic-LDS attribute set through this context
    int    num_cus;            // compute units of the device (hipDeviceAttributeMultiprocessorCount)
    // --- optional per-kernel timing (bbx_profile_enable): hipEvent pairs on the launch stream
    int prof_on, prof_n;
    volatile int prof_gen;     // bumped by bbx_profile_enable / _read
    int prof_open, prof_open_gen, prof_open_idx;
    hipEvent_t* prof_ev;       // [2 * BBX_PROF_MAX]
    int* prof_slot;            // [BBX_PROF_MAX]
};
#define BBX_PROF_MAX 8192
void bbx_prof_start(bbx_ctx* ctx, int slot, hipStream_t s);
void bbx_prof_stop(bbx_ctx* ctx, hipStream_t s);
// single kernels: an event pair that the launch itself stamps (hipExtLaunchKernelGGL) -- begin and end of the kernel's
// execution, without the time the launch waits behind other streams' kernels; (nullptr, nullptr) when profiling is off
void bbx_prof_events(bbx_ctx* ctx, int slot, hipEvent_t* e0, hipEvent_t* e1);
#define BBX_LAUNCH_TIMED(ctx, slot, kern, grid, blk, lds, s, ...)                                   \
    do {                                                                                              \
        hipEvent_t e0_ = nullptr, e1_ = nullptr;                                                      \
        bbx_prof_events(ctx, slot, &e0_, &e1_);                                                       \
        hipExtLaunchKernelGGL(kern, grid, blk, lds, s, e0_, e1_, 0, __VA_ARGS__);                     \
    } while (0)

enum {
    // one 64-byte line per counter: same-line atomics serialise (~11 ns each on MI355X)
    CNT_SAT = 0,          // saturated pixels queued by calibrate
    CNT_CAND = 16,        // LA-Cosmic candidates of the current iteration
    CNT_STAGE2 = 32,      // LA-Cosmic pixels that passed the first growth step
    CNT_CRLIST = 48,      // cumulative CR pixel list
    CNT_NEWCR = 64,       // CR pixels flagged in the current iteration
    CNT_CC_N = 80,        // connected-component scratch: list length
    CNT_CC_ROOTS = 96,    // connected-component scratch: roots
    CNT_TILES = 112,      // fill-holes: unresolved tiles
    CNT_BGNEED = 128,     // LA-Cosmic: pixels that needed the background level
    CNT_TMP = 144,
    CNT_CANDOVF = 160,    // LA-Cosmic candidates that did not fit their tile segment
    CNT_CANDRAW = 176,    // LA-Cosmic candidates before the s > sigclip pre-filter
    CNT_TICKET = 192,     // workgroups of the current kernel that have finished (last one does the epilogue)
    CNT_ZCAND = 208,      // bbx_zogy_frame: pixels with |Scorr| >= the candidate threshold (bbx_zogy_candidates)
    CNT_BCAND = 224,      // bbx_spline_zoom_sub: pixels above the catalogue threshold (bbx_zoom_candidates)
    CNT_BOXFAIL0 = 240,   // bbx_bkg_boxstats: boxes left to the full sort; two counters (CNT_BOXFAIL0, + 1) used by alternate calls
    CNT_MAX = 256
};

// workspace slots
enum {
    WS_HASH = 0, WS_CCLIST, WS_PARENT, WS_BITS_M, WS_BITS_C, WS_BITS_R, WS_TILES,
    WS_CAND, WS_FLAGS, WS_STAGE2, WS_CRLIST, WS_HIST, WS_SEL, WS_MISC, WS_STRIP, WS_HVALS, WS_CRORIG, WS_CANNY, WS_ZCAND, WS_BCAND, WS_FPHINT, WS_BOXFAIL, WS_ZSPL,
    WS_TRANSFIT,
    WS_TRANSSHAPE,       // bbx_trans_shapefit's scalars: a slot of its own, so that the call may be queued beside bbx_trans_psffit's
    WS_LIMFLUX,          // bbx_limflux_image: the windows T_t and the windowed, squared stamps of every tile
    WS_MAX
};
static_assert(WS_MAX <= BBX_WS_SLOTS, "bbx_ctx::d_ws holds BBX_WS_SLOTS slots");

int bbx_hip_fail(bbx_ctx* ctx, hipError_t e, const char* what, int line);
// entries of a candidate pixel list of a frame of npix pixels (bbx_find_peaks and the kernels that list for it: WS_CCLIST,
// WS_ZCAND, WS_BCAND): 1/16 of the frame, as ever, for frames of a million pixels and more; a small frame gets min(npix, 65536)
// entries, so that the star-dense toy frames of the tests fit (a 240 x 480 frame with 300 stars has 3 10^4 pixels above 5 sigma)
static inline size_t bbx_cand_cap(size_t npix) {
    const size_t c = npix / 16 + 1024, f = npix < 65536 ? npix : 65536;
    return c > f ? c : f;
}
void bbx_zogy_frame_release(bbx_ctx* ctx);   // bbx_zogy3.hip: frees ctx->zogy_frame_state (called by bbx_ctx_destroy)
void bbx_fpack_release(bbx_ctx* ctx);     // bbx_fpack.hip: frees the per-stream hint tables (called by bbx_ctx_destroy)
int bbx_build_flags_fpack(void); int bbx_build_flags_zogy(void); int bbx_build_flags_bkg(void); int bbx_build_flags_sat(void); int bbx_build_flags_canny(void);
void bbx_zogy_release(bbx_ctx* ctx);      // bbx_zogy.hip: frees ctx->zogy_state (called by bbx_ctx_destroy)
void* bbx_ws(bbx_ctx* ctx, int slot, size_t bytes, int* rc);

// small per-channel parameter vectors travel as by-value kernel arguments
struct f32x16 { float v[16]; };
struct f64x256 { double v[256]; };

#define BBX_HIP(call)                                                         \
    do {                                                                      \
        hipError_t _e = (call);                                               \
        if (_e != hipSuccess) return bbx_hip_fail(ctx, _e, #call, __LINE__);  \
    } while (0)

#define BBX_LAUNCH_CHECK()                                                    \
    do {                                                                      \
        hipError_t _e = hipGetLastError();                                    \
        if (_e != hipSuccess) return bbx_hip_fail(ctx, _e, "kernel launch", __LINE__); \
    } while (0)

// ---- device helpers -------------------------------------------------------------
// Wave-wide sums, result in every lane.  Inside each 16-lane row the partial sums travel by
// DPP row rotations (plain VALU moves, no LDS crossbar like __shfl/ds_bpermute); the four row
// totals are then read with v_readlane and added in row order.
template <int CTRL> __device__ __forceinline__ int dpp_mov_i32(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false);
}
template <int CTRL> __device__ __forceinline__ float dpp_mov_f32(float v) {
    return __int_as_float(dpp_mov_i32<CTRL>(__float_as_int(v)));
}
template <int CTRL> __device__ __forceinline__ double dpp_mov_f64(double v) {
    const int lo = dpp_mov_i32<CTRL>(__double2loint(v)), hi = dpp_mov_i32<CTRL>(__double2hiint(v));
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double readlane_f64(double v, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}
__device__ __forceinline__ float readlane_f32(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }
#define BBX_DPP_ROR(n) (0x120 + (n))          // row_ror:n
__device__ __forceinline__ double wave_sum_f64(double v) {
    v += dpp_mov_f64<BBX_DPP_ROR(1)>(v);
    v += dpp_mov_f64<BBX_DPP_ROR(2)>(v);
    v += dpp_mov_f64<BBX_DPP_ROR(4)>(v);
    v += dpp_mov_f64<BBX_DPP_ROR(8)>(v);
    return (readlane_f64(v, 0) + readlane_f64(v, 16)) + (readlane_f64(v, 32) + readlane_f64(v, 48));
}
__device__ __forceinline__ float wave_sum_f32(float v) {
    v += dpp_mov_f32<BBX_DPP_ROR(1)>(v);
    v += dpp_mov_f32<BBX_DPP_ROR(2)>(v);
    v += dpp_mov_f32<BBX_DPP_ROR(4)>(v);
    v += dpp_mov_f32<BBX_DPP_ROR(8)>(v);
    return (readlane_f32(v, 0) + readlane_f32(v, 16)) + (readlane_f32(v, 32) + readlane_f32(v, 48));
}
__device__ __forceinline__ int wave_sum_i32(int v) {
    v += dpp_mov_i32<BBX_DPP_ROR(1)>(v);
    v += dpp_mov_i32<BBX_DPP_ROR(2)>(v);
    v += dpp_mov_i32<BBX_DPP_ROR(4)>(v);
    v += dpp_mov_i32<BBX_DPP_ROR(8)>(v);
    return (__builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16)) +
           (__builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48));
}
__device__ __forceinline__ long long wave_sum_i64(long long v) {
    // counts: two 32-bit halves would need carries; the callers' totals fit 2^53 exactly
    return (long long)wave_sum_f64((double)v);
}

// size[root] += 1 for every lane with [on] set, one add per distinct root and wave: neighbours in a pixel list mostly belong
// to the same component, and an add per pixel on the few roots of large components queues up at ~11 ns each.  Called by
// all lanes of the wave
__device__ __forceinline__ void wave_add_per_root(bool on, uint32_t root, uint32_t* size) {
    const int lane = threadIdx.x & 63;
    unsigned long long m = __builtin_amdgcn_ballot_w64(on);
    while (m) {
        const int leader = (int)__builtin_ctzll(m);
        const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)root, leader);
        const unsigned long long same = __builtin_amdgcn_ballot_w64(on && root == r0);
        if (lane == leader) atomicAdd(&size[r0], (unsigned)__popcll(same));
        on = on && root != r0;
        m &= ~same;
    }
}

// neither inf nor NaN: the exponent field is not all ones
__device__ __forceinline__ bool finite_f32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// byte-wide atomic OR through the aligned 32-bit word (little endian)
__device__ __forceinline__ unsigned atomic_or_u8(uint8_t* base, size_t idx, unsigned bits) {
    size_t a = (size_t)(base + idx);
    unsigned* w = (unsigned*)(a & ~(size_t)3);
    unsigned sh = (unsigned)(a & 3) * 8;
    unsigned old = atomicOr(w, bits << sh);
    return (old >> sh) & 0xffu;
}
// ... and its counterpart: clears [bits] of one byte
__device__ __forceinline__ void atomic_clear_u8(uint8_t* base, size_t idx, unsigned bits) {
    size_t a = (size_t)(base + idx);
    atomicAnd((unsigned*)(a & ~(size_t)3), ~(bits << ((unsigned)(a & 3) * 8)));
}

// raw pixel fetch: u16 or f32 -> float
template <int RAW_T>
__device__ __forceinline__ float raw_load(const void* raw, size_t i) {
    if (RAW_T == BBX_RAW_U16) return (float)((const uint16_t*)raw)[i];
    return ((const float*)raw)[i];
}

// float -> order-preserving uint32 key (radix select) and back
__device__ __forceinline__ uint32_t f2key(float f) {
    uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {
    uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return __uint_as_float(u);
}

// ---- a wave sorts 64 * NR keys held NR per lane in registers, ascending: the sorted position of register r of lane l is
// l * NR + r.  Bitonic network: a stage between registers of a lane is v_min / v_max where the element index fixes the
// direction (wave_sort_static: levels of 2 .. NR / 2 elements) and v_med3 against a per-lane 0 / ~0 where the lane does
// (wave_sort_lane: clo = 0 sorts ascending, med3(a, b, 0) = min; ~0 descending); a stage between lanes fetches the partner
// through ds_bpermute (__shfl_xor).
__device__ __forceinline__ uint32_t umed3(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t o;
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(o) : "v"(a), "v"(b), "v"(c));
    return o;
}
template <int NR, int K, int J> __device__ __forceinline__ void wave_sort_static(uint32_t (&k)[NR]) {
#pragma unroll
    for (int r = 0; r < NR; r++) {
        const int q = r ^ J;
        if (q > r) {
            const uint32_t a = k[r], b = k[q];
            const uint32_t lo = min(a, b), hi = max(a, b);
            if ((r & K) == 0) { k[r] = lo; k[q] = hi; } else { k[r] = hi; k[q] = lo; }
        }
    }
}
template <int NR, int J> __device__ __forceinline__ void wave_sort_lane(uint32_t (&k)[NR], uint32_t clo) {
    const uint32_t chi = ~clo;
#pragma unroll
    for (int r = 0; r < NR; r++) {
        const int q = r ^ J;
        if (q > r) {
            const uint32_t a = k[r], b = k[q];
            k[r] = umed3(a, b, clo); k[q] = umed3(a, b, chi);
        }
    }
}
// the two halves of a merge level: every register against lane ^ m (keep the smaller / the larger), then the lane's own
template <int NR> __device__ __forceinline__ void wave_sort_cross(uint32_t (&k)[NR], int lane, int m, bool asc) {
    const uint32_t c = (((lane & m) == 0) == asc) ? 0u : 0xffffffffu;
#pragma unroll
    for (int r = 0; r < NR; r++) k[r] = umed3(k[r], (uint32_t)__shfl_xor((int)k[r], m), c);
}
template <int NR> __device__ __forceinline__ void wave_sort_own(uint32_t (&k)[NR], bool asc) {
    const uint32_t clo = asc ? 0u : 0xffffffffu;
    if constexpr (NR >= 64) wave_sort_lane<NR, 32>(k, clo);
    if constexpr (NR >= 32) wave_sort_lane<NR, 16>(k, clo);
    if constexpr (NR >= 16) wave_sort_lane<NR, 8>(k, clo);
    wave_sort_lane<NR, 4>(k, clo); wave_sort_lane<NR, 2>(k, clo); wave_sort_lane<NR, 1>(k, clo);
}
// NR = 8, 16, 32, 64.  ROLLED keeps the two loops over the merge levels as loops (k_fp_tile, which is long as it is);
// otherwise the compiler decides.  (A pragma cannot depend on a template argument: two loop nests around the same calls.)
template <int NR, bool ROLLED = false> __device__ __forceinline__ void wave_sort(uint32_t (&k)[NR], int lane) {
    static_assert(NR == 8 || NR == 16 || NR == 32 || NR == 64, "wave_sort: 8, 16, 32 or 64 keys per lane");
    wave_sort_static<NR, 2, 1>(k);
    wave_sort_static<NR, 4, 2>(k); wave_sort_static<NR, 4, 1>(k);
    if constexpr (NR >= 16) { wave_sort_static<NR, 8, 4>(k); wave_sort_static<NR, 8, 2>(k); wave_sort_static<NR, 8, 1>(k); }
    if constexpr (NR >= 32) { wave_sort_static<NR, 16, 8>(k); wave_sort_static<NR, 16, 4>(k); wave_sort_static<NR, 16, 2>(k); wave_sort_static<NR, 16, 1>(k); }
    if constexpr (NR >= 64) {
        wave_sort_static<NR, 32, 16>(k); wave_sort_static<NR, 32, 8>(k); wave_sort_static<NR, 32, 4>(k); wave_sort_static<NR, 32, 2>(k);
        wave_sort_static<NR, 32, 1>(k);
    }
    if constexpr (ROLLED) {
#pragma unroll 1
        for (int ll = 0; ll <= 6; ll++) {                 // runs of NR << ll elements
            const bool asc = (lane & (1 << ll)) == 0;     // ll = 6: one ascending run
#pragma unroll 1
            for (int m = (1 << ll) >> 1; m > 0; m >>= 1) wave_sort_cross<NR>(k, lane, m, asc);
            wave_sort_own<NR>(k, asc);
        }
    } else {
        for (int ll = 0; ll <= 6; ll++) {
            const bool asc = (lane & (1 << ll)) == 0;
            for (int m = (1 << ll) >> 1; m > 0; m >>= 1) wave_sort_cross<NR>(k, lane, m, asc);
            wave_sort_own<NR>(k, asc);
        }
    }
}

// ---- workgroup primitives: one LDS sort and the two orders in which the project adds wave totals ----
// compare-exchange of elements i < p of the LDS sort, by element type: min / max with both stores for float (the values are
// not NaN; -0.0 and +0.0 are placed as fminf / fmaxf place them), compare and conditional swap for the integer keys
__device__ __forceinline__ void lds_cswap(float* s, int i, int p, bool asc) {
    const float a = s[i], b = s[p];
    const float lo = fminf(a, b), hi = fmaxf(a, b);
    s[i] = asc ? lo : hi;
    s[p] = asc ? hi : lo;
}
template <typename T> __device__ __forceinline__ void lds_cswap(T* s, int i, int p, bool asc) {
    const T a = s[i], b = s[p];
    if ((a > b) == asc) { s[i] = b; s[p] = a; }
}
// ascending bitonic sort of n = 2^k elements in LDS by the whole workgroup of BLOCK threads (ready for every thread on return)
template <int BLOCK, typename T> __device__ __forceinline__ void lds_sort(T* s, int n) {
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < n / 2; t += BLOCK) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                lds_cswap(s, i, i + j, (i & k) == 0);
            }
            __syncthreads();
        }
}

// Sums of doubles over a workgroup of NW waves, the same values in every thread: wave sums by DPP, the wave totals through LDS.
// The order in which the wave totals are added is part of the pinned bits; there are two, and a call site keeps its own.
// wg_sum_tree: the balanced pairwise tree, (r0 + r1) + (r2 + r3) for four waves.  The two halves of red[N][2][NW] are used
// alternately (ph), so one barrier per call is enough; the half is the inner index, so that calls with different N on one
// buffer (k_thumb_png8: red[Nmax][2][NW]) never write where the call before may still read
template <int NW> __device__ __forceinline__ double wg_tree(const double* r) {
    if constexpr (NW == 1) return r[0];
    else return wg_tree<NW / 2>(r) + wg_tree<NW / 2>(r + NW / 2);
}
template <int NW, int N>
__device__ __forceinline__ void wg_sum_tree(double (&v)[N], double* red, int& ph) {
    static_assert(NW > 0 && (NW & (NW - 1)) == 0, "wg_sum_tree: a power of two of waves");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; k++) v[k] = wave_sum_f64(v[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < N; k++) red[(k * 2 + ph) * NW + wave] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; k++) v[k] = wg_tree<NW>(red + (k * 2 + ph) * NW);
    ph ^= 1;
}
// wg_sum_seq: wave order, ((r0 + r1) + r2) + ...  red[NW][N]; the caller's next use of red is behind a barrier of its own
template <int NW, int N>
__device__ __forceinline__ void wg_sum_seq(double (&v)[N], double* red) {
#pragma unroll
    for (int q = 0; q < N; q++) v[q] = wave_sum_f64(v[q]);
    __syncthreads();                                                 // (red may still be read from the call before)
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < N; q++) red[(threadIdx.x >> 6) * N + q] = v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < N; q++) {
        double t = red[q];
#pragma unroll
        for (int w = 1; w < NW; w++) t += red[w * N + q];
        v[q] = t;
    }
}
template <int NW>
__device__ __forceinline__ double wg_sum_seq(double v, double* red) {
    double a[1] = {v};
    wg_sum_seq<NW, 1>(a, red);
    return a[0];
}

// ---- shared by bbx_psfbuild.hip, bbx_psfphot.hip and bbx_transfit.hip ----
// oracle/coadd.py lanczos3_taps: k(t) = sinc(t) sinc(t / 3) at t = frac - (-2 .. 3), 0 for |t| >= 3, divided by their sum in
// float64, then float32
__device__ __forceinline__ void psb_taps(float frac, float w[6]) {
    const double pi = 3.141592653589793;
    double k[6], s = 0.0;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        const double t = (double)frac - (double)(j - 2);
        const double a = pi * t, b = pi * (t / 3.0);
        double v = (t == 0.0 ? 1.0 : sin(a) / a) * (t == 0.0 ? 1.0 : sin(b) / b);
        if (fabs(t) >= 3.0) v = 0.0;
        k[j] = v; s += v;
    }
#pragma unroll
    for (int j = 0; j < 6; j++) w[j] = (float)(k[j] / s);
}

// ---- shared by bbx_psfphot.hip and bbx_transfit.hip: steps 2 and 3 of bbx_psf_optflux_shift (include/bbx.h) ----
// one pass of the shift by d along one axis of the S x S stamp: out[i] = sum_j w[j] in[i + l + j - 2], in = 0 outside [0, S),
// float32 products added in float32 in tap order.  frac == 0: the taps are the kernel's own limit (0, 0, 1, 0, 0, 0), applied
// as the copy out[i] = in[i + l] that they stand for (no 0 * x, so the pixels keep their bits)
template <bool ALONG_X, int BLOCK>
__device__ __forceinline__ void psb_shift_pass(const float* in, float* out, int S, float d) {
    const float nd = -d, fl = floorf(nd), frac = nd - fl;
    const int l = (int)fl;                                           // (|d| <= 16)
    float w[6];
    psb_taps(frac, w);
    for (int k = threadIdx.x; k < S * S; k += BLOCK) {
        const int r = k / S, c = k - r * S;
        const int pos = (ALONG_X ? c : r) + l;
        const float* line = ALONG_X ? in + r * S : in + c;
        const int step = ALONG_X ? 1 : S;
        float t;
        if (frac == 0.f)
            t = (pos >= 0 && pos < S) ? line[pos * step] : 0.f;
        else {
            t = 0.f;
#pragma unroll
            for (int j = 0; j < 6; j++) {
                const int q = pos + j - 2;
                const float p = (q >= 0 && q < S) ? line[q * step] : 0.f;
                t = j ? t + w[j] * p : w[0] * p;
            }
        }
        out[k] = t;
    }
}
// the stamp in a[S * S] (LDS, behind a barrier) moved by (dy, dx): the row pass (along x) into b, the column pass back into a;
// a is ready for every thread on return
template <int BLOCK>
__device__ __forceinline__ void psb_shift_stamp(float* a, float* b, int S, float dy, float dx) {
    psb_shift_pass<true, BLOCK>(a, b, S, dx);
    __syncthreads();
    psb_shift_pass<false, BLOCK>(b, a, S, dy);
    __syncthreads();
}
// sum of the stamp's pixels in float64: per thread over pixels tid, tid + BLOCK, ..., then wg_sum_seq
template <int BLOCK>
__device__ __forceinline__ double psb_stamp_sum(const float* a, int npx, double* red) {
    double part = 0.0;
    for (int k = threadIdx.x; k < npx; k += BLOCK) part += (double)a[k];
    return wg_sum_seq<BLOCK / 64>(part, red);
}
