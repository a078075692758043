// bbx_zogy3.hip -- ZOGY on whole frames (bbx_zogy_frame): a 2-D FFT pipeline written for this shape.
// Kernel sequence, data layouts (T / U tiles, C coefficient arrays, halo rows) and algebra: DESIGN.md section 4b.
// (The first core of round 2, bbx_zogy2.hip -- lines of 1400 = 35 * 40 points in two steps of register DFTs, one thread per
// sub-transform, ~210 VGPRs, 8 waves per CU, 11.3 ms per frame -- was removed in round 3.)
//
//   1-D transform: L = R0 R1 [R2 [R3]] (1400 = 5 * 7 * 5 * 8); a step is L / R butterflies of radix R
//              per line (decimation in frequency, in place: a butterfly reads and writes the same
//              R positions), any thread takes any butterfly: 45-77 VGPRs, 24 waves per CU, all data
//              movement is loops over the workgroup.  The spectrum is left in the digit-reversed
//              order of the in-place algorithm (pos(k) below); the inverse runs the steps backwards.
//              The butterflies (bbx_fft_gen.h, tools/gen_fft.py) work on (re, im) pairs: packed fp32
//              instructions, the half-crossing operations spelled out with op_sel / neg modifiers.
//
#include "bbx_common.h"
#ifndef Z3_NO_CONTRACT
#pragma clang fp contract(fast)      // the transforms are compared within a tolerance, not bit by bit: let mul + add fuse
#endif
#include "bbx_fft_gen.h"
#include "bbx_spline.h"
#include <math.h>
#include <stdlib.h>

namespace z3 {

struct zscal { float sn, sr, fn, fr, dx, dy; };

// Diagnostic builds only (tools/exp/zvar.sh -DZ3_STAMPS; the Makefile never defines it): thread 0 of every workgroup writes
// the shader clock at the phase boundaries of the kernel into a buffer set by bbx_z3_stamps (tools/dbg/z3_stamps.py).
#ifdef Z3_STAMPS
#define Z3_STAMP_WGS 24576
__device__ unsigned long long* g_z3_stamps;
#define ZSTAMP(kid, i)                                                                                                     \
    do { if (threadIdx.x == 0 && g_z3_stamps && blockIdx.x < Z3_STAMP_WGS)                                                \
            g_z3_stamps[((size_t)(kid) * Z3_STAMP_WGS + blockIdx.x) * 16 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#define ZSTAMP_HEAD(kid)                                                                                                   \
    do { if (threadIdx.x == 0 && g_z3_stamps && blockIdx.x < Z3_STAMP_WGS) {                                              \
            unsigned long long* q_ = g_z3_stamps + ((size_t)(kid) * Z3_STAMP_WGS + blockIdx.x) * 16;                       \
            q_[14] = __builtin_amdgcn_s_memrealtime(); q_[15] = __builtin_amdgcn_s_getreg(((4 - 1) << 11) | (0 << 6) | 20); \
            q_[0] = __builtin_amdgcn_s_memtime(); } } while (0)
#else
#define ZSTAMP(kid, i)
#define ZSTAMP_HEAD(kid)
#endif

constexpr int cmax(int a, int b) { return a > b ? a : b; }
#ifndef Z3_SPREAD
#define Z3_SPREAD 1
#endif
#ifndef Z3_LSMOD
#define Z3_LSMOD (Z3_SPREAD ? 16 : 8)
#endif
constexpr int line_stride(int lp) { int s = lp; while ((2 * s) % 64 != Z3_LSMOD) s++; return s; }

#ifndef Z3_THREADS
#define Z3_THREADS 768         // two workgroups per CU: 24 waves, <= 85 VGPRs (8 parked float2 per thread in the column kernels)
#endif
#ifndef Z3_FIN_THREADS
#define Z3_FIN_THREADS 768     // k_final_rows: 5 lines = 64 KB, two workgroups per CU
#endif
#ifndef Z3_NL
#define Z3_NL 4                // 4 x 4 tiles of float2 = one 128-byte line; LDS: 4 lines = 51 KB per workgroup
#endif
#ifndef Z3_LOADS_T
#define Z3_LOADS_T 4
#endif
#ifndef Z3_LOADS_U
#define Z3_LOADS_U 2
#endif
#ifndef Z3_IMG_LOADS
#define Z3_IMG_LOADS 3
#endif
#ifndef Z3_LIGHT_THREADS
#define Z3_LIGHT_THREADS Z3_THREADS   // k_psf_rows, k_img_rows (nothing parked in registers)
#endif
#ifndef Z3_VAR_THREADS
#define Z3_VAR_THREADS 768     // k_var_cols keeps two spectra in registers: 2 x 8 float2 per thread, 85 VGPRs without spills
#define Z3_VAR_MINW 6          // since the transforms work on (re, im) pairs (512 threads / 128 VGPRs before)
#endif
#ifndef Z3_MINW
#define Z3_MINW 6              // waves per SIMD the register allocation must allow (two workgroups of 768 threads)
#endif
#ifndef Z3_MINW_LIGHT
#define Z3_MINW_LIGHT Z3_MINW  // the same for the kernels without parked registers (k_psf_rows, k_cols_fwd, k_img_rows)
#endif
#ifndef Z3_MINW_PSF
#define Z3_MINW_PSF Z3_MINW
#endif
#ifndef Z3_FIN_MINW
#define Z3_FIN_MINW 6
#endif
#ifndef Z3_PLAN1400
#define Z3_PLAN1400 5, 7, 5, 8
#endif
#ifndef Z3_KWIN_TOL
#define Z3_KWIN_TOL 1e-6       // share of the energy of k_n, k_r (per sub-image) allowed outside the row window: V(S) is off by that share at most
#endif
#ifndef Z3_TWL
#define Z3_TWL 1               // twiddle table in LDS (1) or read from global memory (0: three 8-byte reads per point
                               // and transform through the vector memory path, +9 % on the whole call)
#endif

template <int R0_, int R1_, int R2_ = 1, int R3_ = 1> struct Plan {
    static constexpr int R0 = R0_, R1 = R1_, R2 = R2_, R3 = R3_;
    static constexpr int L = R0_ * R1_ * R2_ * R3_, H = L / 2 + 1;
    static constexpr int NL = L >= 512 ? Z3_NL : 16;                // lines per workgroup
    static constexpr int THREADS = L >= 512 ? Z3_THREADS : 256, FIN_THREADS = L >= 512 ? Z3_FIN_THREADS : 256;
    static constexpr int LIGHT_THREADS = L >= 512 ? Z3_LIGHT_THREADS : 256;
    static constexpr int VAR_THREADS = L >= 512 ? Z3_VAR_THREADS : 256, VAR_MINW = L >= 512 ? Z3_VAR_MINW : 1;
    static constexpr int G = (H + NL - 1) / NL, HP = G * NL;        // column groups, padded half-spectrum width
    static constexpr int LP = L + L / 8 + 1;                        // padded line: one pad per 8 entries
    static constexpr int LS = line_stride(LP);
    static constexpr int LB = (L + NL - 1) / NL;                    // row blocks of NL rows
    static constexpr size_t UNIT = (size_t)LB * NL * HP;            // elements of one T / U / C array per sub-image
    static constexpr int TWL = Z3_TWL;
    static constexpr int MINW_LIGHT = L >= 512 ? Z3_MINW_LIGHT : 1;
    static constexpr int MINW_PSF = L >= 512 ? Z3_MINW_PSF : 1;
    static constexpr int MINW = L >= 512 ? Z3_MINW : 1, FIN_MINW = L >= 512 ? Z3_FIN_MINW : 1;
};

// The matched-filter kernels on a small grid: a plan of side M = L / F with its own line count, and
// which sub-image sides have one.  Of a PlanN only L, H, LP, LS, the radices and NL are used.
template <int NL_, int... R> struct PlanN : Plan<R...> { static constexpr int NL = NL_; };
template <class P> struct small_of { static constexpr bool ok = false; static constexpr int F = 1; typedef P type; };
template <> struct small_of<Plan<5, 7, 5, 8>> { static constexpr bool ok = true; static constexpr int F = 5; typedef PlanN<8, 5, 7, 8> type; };
#define Z3_KS_THREADS 256      // k_ks_cols: 8 lines of 280 points

typedef bbx_v2f __attribute__((may_alias)) v2f_a;     // a float2 of the line buffers read / written as one (re, im) pair
__device__ __forceinline__ bbx_v2f to_v(float2 a) { return bbx_v2f{a.x, a.y}; }
__device__ __forceinline__ float2 from_v(bbx_v2f a) { return make_float2(a.x, a.y); }
__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return from_v(bbx_cmul(to_v(a), to_v(b))); }
__device__ __forceinline__ float2 cmulc(float2 a, float2 b) { return from_v(bbx_cmulc(to_v(a), to_v(b))); }   // a * conj(b)
__device__ __forceinline__ float2 cscale(float2 a, float s) { return make_float2(a.x * s, a.y * s); }

// Streaming accesses of the big arrays (frames, T / U tiles, the PSF spectra: written once, read once, 0.5 GB each): non-temporal.
// Measured with the kernels' own access shape (tools/exp/tile_bw.hip: a workgroup reads 350 pieces of 128 bytes at a 22.5 KB
// stride and writes 45 KB contiguously, 2 workgroups per CU): plain loads + plain stores 3.5 TB/s, plain loads + non-temporal
// stores 6.1, both non-temporal 6.9 (a contiguous copy of the same shape: 5.9) -- plain stores keep their lines in the
// XCD's L2 and push out the lines the scattered reads still need.
#ifndef Z3_NT
#define Z3_NT 1
#endif
typedef float z3_v4 __attribute__((ext_vector_type(4)));
typedef float z3_v2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float4 ld_nt(const float4* p) {
#if Z3_NT
    const z3_v4 v = __builtin_nontemporal_load(reinterpret_cast<const z3_v4*>(p)); return make_float4(v.x, v.y, v.z, v.w);
#else
    return *p;
#endif
}
__device__ __forceinline__ float2 ld_nt(const float2* p) {
#if Z3_NT
    const z3_v2 v = __builtin_nontemporal_load(reinterpret_cast<const z3_v2*>(p)); return make_float2(v.x, v.y);
#else
    return *p;
#endif
}
__device__ __forceinline__ void st_nt(float4* p, float4 v) {
#if Z3_NT
    __builtin_nontemporal_store(z3_v4{v.x, v.y, v.z, v.w}, reinterpret_cast<z3_v4*>(p));
#else
    *p = v;
#endif
}
__device__ __forceinline__ void st_nt(float2* p, float2 v) {
#if Z3_NT
    __builtin_nontemporal_store(z3_v2{v.x, v.y}, reinterpret_cast<z3_v2*>(p));
#else
    *p = v;
#endif
}
__device__ __forceinline__ void st_nt(float* p, float v) {
#if Z3_NT
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}

__device__ __forceinline__ int npos(int n) { return n + (n >> 3); }                       // LDS position of entry n of a line
// position of spectral index k after the forward transform (digit reversal of the in-place passes)
template <class P> __device__ __forceinline__ int ppos(int k) {
    int p = (k % P::R0) * (P::L / P::R0); k /= P::R0;
    p += (k % P::R1) * (P::L / (P::R0 * P::R1)); k /= P::R1;
    if (P::R2 > 1) { p += (k % P::R2) * (P::L / (P::R0 * P::R1 * P::R2)); k /= P::R2; }
    if (P::R3 > 1) p += k;
    return npos(p);
}
// spectral index at position p of a line (before the padding): the inverse of ppos
template <class P> __device__ __forceinline__ int kofp(int p) {
    constexpr int S0 = P::L / P::R0, S1 = S0 / P::R1, S2 = S1 / P::R2;
    int k = p / S0; p -= k * S0;
    k += P::R0 * (p / S1); p %= S1;
    if (P::R2 > 1) { k += P::R0 * P::R1 * (p / S2); p %= S2; }
    if (P::R3 > 1) k += P::R0 * P::R1 * P::R2 * p;
    return k;
}

// one radix-R pass over blocks of B entries of NLINES lines (B / R = M butterflies per block).  (A thread taking the same
// butterfly of two neighbouring lines -- positions and twiddles worked out once for both -- needs ~50 more registers than
// the 85 that two workgroups of 768 threads leave: it spills and is 15 % slower.)  The
// butterfly's R positions are base + r M: with the padding they stay an affine function of r when M
// is a multiple of 8, or when M = 1 and the block starts at a multiple of 8 (constant offsets).
template <class P, int R, int B, bool INV, int NLINES, int ZP = 0>
__device__ __forceinline__ void fft_step(float2* s, const float2* __restrict__ tw, int zw = 0) {
    constexpr int M = B / R, PER = P::L / R, NTASK = NLINES * PER, TWS = P::L / B;
    constexpr bool AFF8 = M % 8 == 0, AFF1 = M == 1 && (8 % R == 0 || R % 8 == 0);
    // Lanes -> butterflies.  SPREAD (M a multiple of 8, groups of 4 lines): 8 consecutive lanes take 8 consecutive
    // butterflies of one line, the next 8 lanes the same butterflies of the next line.  With the line stride = 8 entries
    // mod 32 the 32 lanes one ds_read_b64 group serves then touch 32 different 8-byte banks (a run of 32 consecutive
    // entries of ONE line covers 35 padded positions: a two-way conflict on every read), and their twiddle reads are the
    // same 8 addresses for the 4 lines.
    constexpr bool SPREAD = Z3_SPREAD && AFF8 && PER % 8 == 0 && NLINES >= 4;
    constexpr int NSPREAD = SPREAD ? (NLINES / 4) * 4 * PER : 0;
    for (int task = threadIdx.x; task < NTASK; task += blockDim.x) {
        int l, j;
        if (SPREAD && task < NSPREAD) {
            const int lg = NLINES >= 8 ? task / (4 * PER) : 0, t = task - lg * (4 * PER);
            l = lg * 4 + ((t >> 3) & 3); j = ((t >> 5) << 3) | (t & 7);
        } else { l = task / PER; j = task - l * PER; }
        const int b = j / M, m = j - b * M;
        // lines that are zero outside their first and last [zw] entries (PSF stamps, windowed kernels): a butterfly of the
        // first pass (ZP 1) or the second (ZP 2) whose inputs all lie in the zero stretch leaves its zeros as they are
        if (ZP == 1 && zw > 0 && m >= zw && m < M - zw) continue;
        if (ZP == 2 && zw > 0 && m >= zw && m + (R - 1) * M < B - zw) continue;
        const int base = b * B + m;
        v2f_a* line = reinterpret_cast<v2f_a*>(s + l * P::LS + ((AFF8 || AFF1) ? npos(base) : 0));
        const v2f_a* twv = reinterpret_cast<const v2f_a*>(tw);
        bbx_v2f u[R];
#pragma unroll
        for (int r = 0; r < R; r++) u[r] = line[AFF8 ? r * (M + M / 8) : AFF1 ? r + r / 8 : npos(base + r * M)];
        // twiddles W^(m k TWS), k = 1 .. R-1: one table read, the powers by multiplication (Z3_TWPOW), or R-1 reads
        bbx_v2f w[R];
        if constexpr (M > 1) {
#ifdef Z3_TWPOW
            w[1] = twv[m * TWS];
#pragma unroll
            for (int k = 2; k < R; k++) w[k] = (k % 2 == 0) ? bbx_cmul(w[k / 2], w[k / 2]) : bbx_cmul(w[k - 1], w[1]);
#else
#pragma unroll
            for (int k = 1; k < R; k++) w[k] = twv[m * k * TWS];
#endif
        }
        if (!INV) {
            bbx_dft<R>::fwd(u);
            if constexpr (M > 1) {
#pragma unroll
                for (int k = 1; k < R; k++) u[k] = bbx_cmul(u[k], w[k]);
            }
        } else {
            if constexpr (M > 1) {
#pragma unroll
                for (int k = 1; k < R; k++) u[k] = bbx_cmulc(u[k], w[k]);
            }
            bbx_dft<R>::inv(u);
        }
#pragma unroll
        for (int r = 0; r < R; r++) line[AFF8 ? r * (M + M / 8) : AFF1 ? r + r / 8 : npos(base + r * M)] = u[r];
    }
}
// forward: natural order -> spectrum at ppos; inverse: back (unnormalised).  Barriers after every pass.
// (zw > 0: the lines are exactly zero outside their first and last zw entries)
template <class P, int NLINES = P::NL> __device__ __forceinline__ void fft_fwd(float2* s, const float2* tw, int zw = 0) {
#ifdef Z3_SKIP_FFT
    __syncthreads(); return;
#endif
#ifdef Z3_NO_ZSKIP
    zw = 0;
#endif
    fft_step<P, P::R0, P::L, false, NLINES, 1>(s, tw, zw); __syncthreads();
    fft_step<P, P::R1, P::L / P::R0, false, NLINES, 2>(s, tw, zw); __syncthreads();
    if constexpr (P::R2 > 1) { fft_step<P, P::R2, P::L / (P::R0 * P::R1), false, NLINES>(s, tw); __syncthreads(); }
    if constexpr (P::R3 > 1) { fft_step<P, P::R3, P::L / (P::R0 * P::R1 * P::R2), false, NLINES>(s, tw); __syncthreads(); }
}
template <class P, int NLINES = P::NL> __device__ __forceinline__ void fft_inv(float2* s, const float2* tw) {
#ifdef Z3_SKIP_FFT
    __syncthreads(); return;
#endif
    if constexpr (P::R3 > 1) { fft_step<P, P::R3, P::L / (P::R0 * P::R1 * P::R2), true, NLINES>(s, tw); __syncthreads(); }
    if constexpr (P::R2 > 1) { fft_step<P, P::R2, P::L / (P::R0 * P::R1), true, NLINES>(s, tw); __syncthreads(); }
    fft_step<P, P::R1, P::L / P::R0, true, NLINES>(s, tw); __syncthreads();
    fft_step<P, P::R0, P::L, true, NLINES>(s, tw); __syncthreads();
}

// per-workgroup tables behind the line buffers: the twiddles (LDS copy, or the global table) and the
// position of every spectral index (ppos costs ~25 VALU instructions; the packing / splitting loops need two per entry)
struct aux_t { const float2* tw; const unsigned short* pp; };
template <class P> __device__ __forceinline__ aux_t aux_setup(float2* after_lines, const float2* __restrict__ twg) {
    aux_t a;
    a.tw = twg;
    if (P::TWL) {
        for (int e = threadIdx.x; e < P::L; e += blockDim.x) after_lines[e] = twg[e];
        a.tw = after_lines;
        after_lines += P::L;
    }
    unsigned short* pp = reinterpret_cast<unsigned short*>(after_lines);
    for (int e = threadIdx.x; e < P::L; e += blockDim.x) pp[e] = (unsigned short)ppos<P>(e);
    a.pp = pp;
    return a;                                                       // visible after the caller's next barrier
}
template <class P> constexpr size_t aux_bytes() { return (P::TWL ? (size_t)P::L * sizeof(float2) : 0) + (((size_t)P::L * 2 + 15) & ~(size_t)15); }

// Workgroup -> (x, y) of an nx * ny task grid, launched as a 1-D grid of a multiple of 8 workgroups.
// Workgroups are dealt round-robin over the 8 XCDs (observed, for speed only): the tasks are numbered so
// that the ones an XCD runs at the same time are neighbours -- they read adjacent 288-byte pieces
// of the same 128-byte lines, which then come from that XCD's L2 instead of HBM a second time.
#ifndef Z3_NO_XCD
__device__ __forceinline__ int xcd_task() { return (int)(blockIdx.x % 8) * (int)(gridDim.x / 8) + (int)(blockIdx.x / 8); }
#else
__device__ __forceinline__ int xcd_task() { return (int)blockIdx.x; }
#endif
#define WG_TASK(nx_, ny_, x_, y_)                       \
    const int task_ = xcd_task();                       \
    if (task_ >= (nx_) * (ny_)) return;                 \
    const int x_ = task_ % (nx_), y_ = task_ / (nx_);
// The row kernels (image cut -> T tiles, U tiles -> output frames) take their tasks in launch order: their neighbours share
// no lines (a task reads and writes whole rows of its own), and the XCD-aware order costs them 1-4 % (measured, round 3).
#ifndef Z3_ROWS_XCD
#define WG_TASK_ROWS(nx_, ny_, x_, y_)                  \
    const int task_ = (int)blockIdx.x;                  \
    if (task_ >= (nx_) * (ny_)) return;                 \
    const int x_ = task_ % (nx_), y_ = task_ / (nx_);
#else
#define WG_TASK_ROWS WG_TASK
#endif
static inline dim3 grid8(int nx, int ny) { return dim3((unsigned)(((size_t)nx * ny + 7) / 8 * 8)); }

// ---- data movement (loops over the workgroup) ---------------------------------------------------
// The final kernel's workgroups take chunks of consecutive row blocks of one sub-image: chunk c of nch covers the blocks
// start[c] .. start[c + 1] - 1 (the same cut for every sub-image; host: chunk_plan); only the row above a chunk's first block
// travels through the halo arrays H[sub][c][HP] (inside a chunk the row above a block is the last row of the block before
// it, still in LDS).
struct chunk_args { const int* start; int nch; };
__device__ __forceinline__ int chunk_start(const chunk_args& ch, int c) { return ch.start[c]; }
// LDS (natural order, after an inverse column pass) -> U tiles U[sub][g][y][l]; halo rows on request
template <class P> __device__ __forceinline__ void store_u(const float2* s, float2* __restrict__ U, int sub, int g, float2* __restrict__ halo = nullptr,
                                                            chunk_args ch = chunk_args{nullptr, 0}) {
    float2* base = U + (size_t)sub * P::UNIT + (size_t)g * P::L * P::NL;
    // two neighbouring lines per item: one 16-byte store
    constexpr int HL = P::NL / 2;
    for (int e = threadIdx.x; e < P::L * HL; e += blockDim.x) {
        const int y = e / HL, l = 2 * (e - y * HL), py = npos(y);
        const float2 v0 = s[l * P::LS + py], v1 = s[(l + 1) * P::LS + py];
        st_nt(reinterpret_cast<float4*>(base + (size_t)y * P::NL + l), make_float4(v0.x, v0.y, v1.x, v1.y));
    }
    if (halo) {
        for (int e = threadIdx.x; e < ch.nch * HL; e += blockDim.x) {
            const int c = e / HL, l = 2 * (e - c * HL), yb = chunk_start(ch, c);
            const int y = yb ? yb * P::NL - 1 : P::L - 1, py = npos(y);                    // row L - 1 above row 0: np.roll
            const float2 v0 = s[l * P::LS + py], v1 = s[(l + 1) * P::LS + py];
            *reinterpret_cast<float4*>(halo + ((size_t)sub * ch.nch + c) * P::HP + g * P::NL + l) = make_float4(v0.x, v0.y, v1.x, v1.y);
        }
    }
}
// The matched-filter kernels k_n, k_r live around the origin: of the inverse column pass of k^ only the rows
// y < wh and y >= L - wh leave the workgroup (U tiles, same layout; the other rows are never read).  The energy
// the dropped rows hold is summed next to the total (Parseval along x: row y of this half spectrum carries
// sum_x k(y, x)^2), so that the host-chosen window can be checked on the device.
template <class P> __device__ __forceinline__ void store_u_win(const float2* s, float2* __restrict__ U, int sub, int g, int wh, double& e_all, double& e_out) {
    float2* base = U + (size_t)sub * P::UNIT + (size_t)g * P::L * P::NL;
    constexpr int HL = P::NL / 2;
    float ea = 0.f, eo = 0.f;
    for (int e = threadIdx.x; e < P::L * HL; e += blockDim.x) {
        const int y = e / HL, l = 2 * (e - y * HL), py = npos(y);
        const float2 v0 = s[l * P::LS + py], v1 = s[(l + 1) * P::LS + py];
        const float en = (v0.x * v0.x + v0.y * v0.y) + (v1.x * v1.x + v1.y * v1.y);
        ea += en;
        if (y < wh || y >= P::L - wh) st_nt(reinterpret_cast<float4*>(base + (size_t)y * P::NL + l), make_float4(v0.x, v0.y, v1.x, v1.y));
        else eo += en;
    }
    e_all += (double)ea; e_out += (double)eo;
}
// T tiles of the row blocks inside the window (rows < wh and >= L - wh; wh a multiple of NL, L a multiple of NL) of
// column group g -> LDS lines; the rows outside the window are zero
template <class P> __device__ __forceinline__ void load_t_lines_win(const float2* T, int sub, int g, float2* s, int wh) {
    const float2* src = T + (size_t)sub * P::UNIT + (size_t)g * P::NL * P::NL;
    constexpr int TV = P::NL * P::NL / 2;
    const int wb = wh / P::NL, NVW = 2 * wb * TV;
    for (int e = threadIdx.x; e < P::NL * (P::L - 2 * wh); e += blockDim.x) {
        const int l = e / (P::L - 2 * wh), y = wh + e - l * (P::L - 2 * wh);
        s[l * P::LS + npos(y)] = make_float2(0.f, 0.f);
    }
    for (int e = threadIdx.x; e < NVW; e += blockDim.x) {
        const int ybw = e / TV, j = e - ybw * TV, yb = ybw < wb ? ybw : P::LB - 2 * wb + ybw;
        const float4 v = ld_nt(reinterpret_cast<const float4*>(src + (size_t)yb * P::HP * P::NL + 2 * j));
        const int l = (2 * j) / P::NL, y = yb * P::NL + (2 * j) % P::NL;
        float2* line = s + l * P::LS;
        line[npos(y)] = make_float2(v.x, v.y); line[npos(y + 1)] = make_float2(v.z, v.w);
    }
}
// T tiles T[sub][yb][kx][yi] of column group g -> LDS lines, natural order
template <class P> __device__ __forceinline__ void load_t_lines(const float2* T, int sub, int g, float2* s) {
    static_assert(P::NL % 2 == 0 && P::L % 2 == 0, "even tile side and line length");
    const float2* src = T + (size_t)sub * P::UNIT + (size_t)g * P::NL * P::NL;
    constexpr int TV = P::NL * P::NL / 2, NV = P::LB * TV;          // float4 per tile, per workgroup
    constexpr int TD = Z3_LOADS_T;                                  // 16-byte loads in flight per thread
    for (int e0 = threadIdx.x; e0 < NV; e0 += TD * (int)blockDim.x) {
        float4 v[TD];
#pragma unroll
        for (int i = 0; i < TD; i++) {
            const int e = e0 + i * (int)blockDim.x;
            if (e < NV) { const int yb = e / TV, j = e - yb * TV; v[i] = ld_nt(reinterpret_cast<const float4*>(src + (size_t)yb * P::HP * P::NL + 2 * j)); }
        }
#pragma unroll
        for (int i = 0; i < TD; i++) {
            const int e = e0 + i * (int)blockDim.x;
            if (e < NV) {
                const int yb = e / TV, j = e - yb * TV, l = (2 * j) / P::NL, y = yb * P::NL + (2 * j) % P::NL;
                if (y < P::L) {
                    float2* line = s + l * P::LS;
                    line[npos(y)] = make_float2(v[i].x, v[i].y); line[npos(y + 1)] = make_float2(v[i].z, v[i].w);
                }
            }
        }
    }
}
template <class P> __device__ __forceinline__ void pack_store(float2* line, const unsigned short* pp, int kx, float2 a, float2 b) {
    if (kx >= P::H) return;
    line[pp[kx]] = make_float2(a.x - b.y, a.y + b.x);
    if (kx >= 1 && P::L - kx >= P::H) line[pp[P::L - kx]] = make_float2(a.x + b.y, b.x - a.y);
}
// Hermitian packing of two U half spectra (row block yb) into full complex lines in spectrum order: Z = a + i b
template <class P> __device__ __forceinline__ void load_u_pair(const float2* __restrict__ Ua, const float2* __restrict__ Ub, int sub, int yb, float2* s,
                                                                const unsigned short* pp) {
    constexpr int TV = P::NL * P::NL / 2, NV = P::G * TV;
    const size_t base = (size_t)sub * P::UNIT + (size_t)yb * P::NL * P::NL;
    constexpr int UD = Z3_LOADS_U;                                  // pairs of 16-byte loads in flight per thread
    for (int e0 = threadIdx.x; e0 < NV; e0 += UD * (int)blockDim.x) {
        float4 va[UD], vb[UD];
#pragma unroll
        for (int i = 0; i < UD; i++) {
            const int e = e0 + i * (int)blockDim.x;
            if (e < NV) {
                const int g = e / TV, j = e - g * TV;
                const size_t o = base + (size_t)g * P::L * P::NL + 2 * j;
                va[i] = ld_nt(reinterpret_cast<const float4*>(Ua + o)); vb[i] = ld_nt(reinterpret_cast<const float4*>(Ub + o));
            }
        }
#pragma unroll
        for (int i = 0; i < UD; i++) {
            const int e = e0 + i * (int)blockDim.x;
            if (e < NV) {
                const int g = e / TV, j = e - g * TV, row = (2 * j) / P::NL, l = (2 * j) % P::NL;      // tile entry [row][l], l even
                if (yb * P::NL + row < P::L) {
                    float2* line = s + row * P::LS;
                    pack_store<P>(line, pp, g * P::NL + l, make_float2(va[i].x, va[i].y), make_float2(vb[i].x, vb[i].y));
                    pack_store<P>(line, pp, g * P::NL + l + 1, make_float2(va[i].z, va[i].w), make_float2(vb[i].z, vb[i].w));
                }
            }
        }
    }
}
template <class P> __device__ __forceinline__ void load_halo_pair(const float2* __restrict__ Ha, const float2* __restrict__ Hb, int sub, int yb, float2* line,
                                                                   const unsigned short* pp) {
    const size_t base = ((size_t)sub * P::LB + yb) * P::HP;
    for (int kx = threadIdx.x; kx < P::H; kx += blockDim.x) pack_store<P>(line, pp, kx, Ha[base + kx], Hb[base + kx]);
}
// The same loads split in two: all of a workgroup's 16-byte loads into registers first (issued before a
// transform of other data, so that their latency hides behind it), the LDS stores later.
template <class P, int T> struct t_regs { static constexpr int N = (P::LB * P::NL * P::NL / 2 + T - 1) / T; float4 v[N]; };
// (I0, I1: the part of a thread's loads to issue / store; a kernel short of registers takes the rest in a second round)
template <class P, int T, int I0 = 0, int I1 = 1 << 30> __device__ __forceinline__ void fetch_t_lines(const float2* __restrict__ Tin, int sub, int g, t_regs<P, T>& r) {
    const float2* src = Tin + (size_t)sub * P::UNIT + (size_t)g * P::NL * P::NL;
    constexpr int TV = P::NL * P::NL / 2, NV = P::LB * TV;
#pragma unroll
    for (int i = I0; i < (I1 < t_regs<P, T>::N ? I1 : t_regs<P, T>::N); i++) {
        const int e = (int)threadIdx.x + i * T;
        if (e < NV) { const int yb = e / TV, j = e - yb * TV; r.v[i] = ld_nt(reinterpret_cast<const float4*>(src + (size_t)yb * P::HP * P::NL + 2 * j)); }
    }
}
template <class P, int T, int I0 = 0, int I1 = 1 << 30> __device__ __forceinline__ void pack_t_lines(const t_regs<P, T>& r, float2* s) {
    constexpr int TV = P::NL * P::NL / 2, NV = P::LB * TV;
#pragma unroll
    for (int i = I0; i < (I1 < t_regs<P, T>::N ? I1 : t_regs<P, T>::N); i++) {
        const int e = (int)threadIdx.x + i * T;
        if (e < NV) {
            const int yb = e / TV, j = e - yb * TV, l = (2 * j) / P::NL, y = yb * P::NL + (2 * j) % P::NL;
            if (y < P::L) {
                float2* line = s + l * P::LS;
                line[npos(y)] = make_float2(r.v[i].x, r.v[i].y); line[npos(y + 1)] = make_float2(r.v[i].z, r.v[i].w);
            }
        }
    }
}
template <class P, int T> struct u_regs { static constexpr int N = (P::G * P::NL * P::NL / 2 + T - 1) / T; float4 a[N], b[N]; };
template <class P, int T> __device__ __forceinline__ void fetch_u_pair(const float2* __restrict__ Ua, const float2* __restrict__ Ub, int sub, int yb,
                                                                        u_regs<P, T>& r, int tid = (int)threadIdx.x) {
    constexpr int TV = P::NL * P::NL / 2, NV = P::G * TV;
    const size_t base = (size_t)sub * P::UNIT + (size_t)yb * P::NL * P::NL;
#pragma unroll
    for (int i = 0; i < u_regs<P, T>::N; i++) {
        const int e = tid + i * T;
        if (e < NV) {
            const int g = e / TV, j = e - g * TV;
            const size_t o = base + (size_t)g * P::L * P::NL + 2 * j;
            r.a[i] = ld_nt(reinterpret_cast<const float4*>(Ua + o)); r.b[i] = ld_nt(reinterpret_cast<const float4*>(Ub + o));
        }
    }
}
template <class P, int T> __device__ __forceinline__ void pack_u_pair(const u_regs<P, T>& r, int yb, float2* s, const unsigned short* pp,
                                                                       int tid = (int)threadIdx.x) {
    constexpr int TV = P::NL * P::NL / 2, NV = P::G * TV;
#pragma unroll
    for (int i = 0; i < u_regs<P, T>::N; i++) {
        const int e = tid + i * T;
        if (e < NV) {
            const int g = e / TV, j = e - g * TV, row = (2 * j) / P::NL, l = (2 * j) % P::NL;
            if (yb * P::NL + row < P::L) {
                float2* line = s + row * P::LS;
                pack_store<P>(line, pp, g * P::NL + l, make_float2(r.a[i].x, r.a[i].y), make_float2(r.b[i].x, r.b[i].y));
                pack_store<P>(line, pp, g * P::NL + l + 1, make_float2(r.a[i].z, r.a[i].w), make_float2(r.b[i].z, r.b[i].w));
            }
        }
    }
}
// Hermitian split of a packed transform Z (LDS, spectrum order) -> two half spectra, T tiles of row block yb
template <class P> __device__ __forceinline__ void store_t_split(const float2* s, const unsigned short* pp, float2* __restrict__ Ta, float2* __restrict__ Tb, int sub,
                                                                  int yb) {
    const size_t base = (size_t)sub * P::UNIT + (size_t)yb * P::HP * P::NL;         // the block's entries (kx, row) are contiguous
    // a thread takes a column kx for all rows of the block: one pair of positions, NL / 2 16-byte stores per output array
    for (int kx = threadIdx.x; kx < P::H; kx += blockDim.x) {
        const int pk = pp[kx], pm = pp[kx ? P::L - kx : 0];
        float4* ta = reinterpret_cast<float4*>(Ta + base + (size_t)kx * P::NL);
        float4* tb = reinterpret_cast<float4*>(Tb + base + (size_t)kx * P::NL);
#pragma unroll
        for (int r = 0; r < P::NL; r += 2) {
            const float2 zk0 = s[r * P::LS + pk], zm0 = s[r * P::LS + pm], zk1 = s[(r + 1) * P::LS + pk], zm1 = s[(r + 1) * P::LS + pm];
            st_nt(ta + r / 2, make_float4(0.5f * (zk0.x + zm0.x), 0.5f * (zk0.y - zm0.y), 0.5f * (zk1.x + zm1.x), 0.5f * (zk1.y - zm1.y)));
            st_nt(tb + r / 2, make_float4(0.5f * (zk0.y + zm0.y), 0.5f * (zm0.x - zk0.x), 0.5f * (zk1.y + zm1.y), 0.5f * (zm1.x - zk1.x)));
        }
    }
}
// spectrum entry e = l * L + p of the C layout <-> LDS
// the same loop with a per-thread register array alongside: iteration k of thread t is entry e = t + k THREADS,
// every time, so a value parked in reg[k] meets the same entry again
// (the thread index goes through an empty asm so that the 17 entry addresses are recomputed in every
// loop instead of being kept in registers across the transforms in between)
__device__ __forceinline__ int opaque_tid() { int t = (int)threadIdx.x; asm volatile("" : "+v"(t)); return t; }
// entry e -> (line l, position p).  With 4 lines of a multiple of 8 entries: 8 consecutive entries of one line, then the
// same 8 of the next line (as the butterflies of fft_step: the 32 lanes of a read group touch 32 different banks).  The
// C arrays are stored in this order of e, by the same loops.
template <class P> __device__ __forceinline__ void e2lp(int e, int& l, int& p) {
    if constexpr (Z3_SPREAD && P::NL == 4 && P::L % 8 == 0) { l = (e >> 3) & 3; p = ((e >> 5) << 3) | (e & 7); }
    else { l = e / P::L; p = e - l * P::L; }
}
#define R_LOOP(k, e, l, p)                                                                     \
    for (int t_ = opaque_tid(), once_ = 1; once_; once_ = 0)                                     \
    _Pragma("unroll") for (int k = 0, e, l, p; k < NE; k++)                                      \
        if (e = t_ + k * RT, e2lp<P>(e, l, p), e < P::NL * P::L)                      /* RT: the kernel's thread count */
#define C_LOOP(e, l, p) for (int e = threadIdx.x, l, p; e2lp<P>(e, l, p), e < P::NL * P::L; e += blockDim.x)

// V(S)^ is scaled by a power of two before it shares a transform with D (float32 rounding leaks ~1e-7 of the larger part of a
// complex transform into the smaller; the scale, chosen per sub-image from Parseval sums of k^2, is exact to undo)
__device__ __forceinline__ float vs_scale_of(double a, double b, const zscal& z, double n2) {
    const float level = (float)(((double)z.sn * z.sn * a + (double)z.sr * z.sr * b) / n2);            // Parseval: sum_x k^2 = sum_k |k^|^2 / L^2
    if (!(level > 0.f) || !isfinite(level)) return 1.f;
    return exp2f(-rintf(log2f(level)));
}
// The per-sub-image scalars every later workgroup needs -- F_S, the scale of V(S)^ and its inverse -- from k_psf_cols'
// partial sums, and the check of the row window: one wave per sub-image (first workgroup of k_psf_rows; rounds 3-4: a
// serial loop over the G partial sums in thread 0 of every workgroup of k_var_cols and k_final_rows).
struct sub_scal { float fs, beta, ibeta, pad; };
template <class P> __device__ __forceinline__ void sub_scalars(const double* __restrict__ fs_partial, int nsub, int sub, const zscal& z, bool win,
                                                                sub_scal* __restrict__ out, int32_t* __restrict__ d_err) {
    // lanes 0 .. 63 of one wave
    const int lane = (int)(threadIdx.x & 63);
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int g = lane; g < P::G; g += 64) {
#pragma unroll
        for (int i = 0; i < 5; i++) if (i < 3 || win) v[i] += fs_partial[((size_t)i * nsub + sub) * P::G + g];
    }
#pragma unroll
    for (int i = 0; i < 5; i++) v[i] = wave_sum_f64(v[i]);
    if (lane == 0) {
        const double n2 = (double)P::L * (double)P::L;
        sub_scal r;
        r.fs = (float)(v[0] / n2);
        r.beta = vs_scale_of(v[1], v[2], z, n2);
        r.ibeta = 1.0f / r.beta; r.pad = 0.f;
        out[sub] = r;
        // the rows the window dropped from k_n, k_r must hold nothing a float32 transform could tell from zero
        if (win && !(v[4] <= Z3_KWIN_TOL * v[3])) atomicOr(d_err, BBX_DERR_PSF_WINDOW);
    }
}

// ---- PSF side ---------------------------------------------------------------------------------
// Row DFT of the S non-zero rows of every PSF stamp, summed directly: Q[which][sub][j][kx] = sum_x p[j][x] W^(kx (x - h)),
// kx < H (the stamp's columns sit at x = -h .. S-1-h mod L).  A thread takes one kx and ZQ_J stamp rows: the twiddle of a
// column is read once for all of them, the stamp values are wave-uniform.  (Round 5: this sum sat inside k_psf_cols, one
// L2 round trip per four terms in every workgroup: 2 x 11 000 of its 75 000 cycles.)
#define ZQ_J 7
template <class P>
__global__ __launch_bounds__(256) void k_psf_rowdft(const float* __restrict__ psf_n, const float* __restrict__ psf_r, int S, const float2* __restrict__ twg,
                                                    float2* __restrict__ Q, int nsub) {
    __shared__ float2 tw[P::L];
    for (int e = threadIdx.x; e < P::L; e += blockDim.x) tw[e] = twg[e];
    __syncthreads();
    const int kx = (int)(blockIdx.x * blockDim.x + threadIdx.x), j0 = (int)blockIdx.y * ZQ_J;
    const int which = (int)blockIdx.z / nsub, sub = (int)blockIdx.z - which * nsub;
    if (kx >= P::H) return;
    const float* st = (which ? psf_r : psf_n) + (size_t)sub * S * S;
    const int h = S / 2;
    float2 acc[ZQ_J];
#pragma unroll
    for (int jj = 0; jj < ZQ_J; jj++) acc[jj] = make_float2(0.f, 0.f);
    int idx = (kx * ((P::L - h % P::L) % P::L)) % P::L;             // kx (L - h) < H L: 32-bit
    for (int x = 0; x < S; x++) {
        const float2 w = tw[idx];
#pragma unroll
        for (int jj = 0; jj < ZQ_J; jj++) {
            if (j0 + jj < S) { const float pv = st[(j0 + jj) * S + x]; acc[jj].x += pv * w.x; acc[jj].y += pv * w.y; }
        }
        idx += kx; if (idx >= P::L) idx -= P::L;
    }
#pragma unroll
    for (int jj = 0; jj < ZQ_J; jj++)
        if (j0 + jj < S) Q[(((size_t)which * nsub + sub) * S + (j0 + jj)) * P::HP + kx] = acc[jj];
}

// KS (small grid): k_n^, k_r^ are not taken back to real space here.  Their entries with ky and kx multiples of F go to the
// half spectra of the small grid, Ukr[sub][which][kx / F][ky / F] (which: 0 k_r^, 1 k_n^; Ukn then holds the cells of the window
// check, zeroed here); k_ks_cols and k_ks_rows take them from there.
// PREP (prepared reference PSF, bbx_zogy_refpsf; full-grid path -- on the small-grid path k_img_cols does this kernel's work):
// Q holds the new stamps' row DFTs only and one pass (Pn^) runs; Pr^ comes from the prepared buffer cPr (C layout,
// k_refpsf_cols: the bits pass 1 would make), a thread's entries loaded into registers behind the transform; cP is then a
// float2 array that takes Pn^ alone.
template <class P, bool KS, bool PREP = false>
__global__ __launch_bounds__(P::THREADS, P::MINW_PSF) void k_psf_cols(const float2* __restrict__ Q, int S,
                                                         const zscal* __restrict__ sc, const float2* __restrict__ twg,
                                                         float4* __restrict__ cP, const float2* __restrict__ cPr,
                                                         float2* __restrict__ Ukn, float2* __restrict__ Ukr,
                                                         double* __restrict__ fs_partial, int nsub, int wh) {
    extern __shared__ float2 s[];
    __shared__ double red[5][P::THREADS / 64];
    if (KS && blockIdx.x == 0) {
        float* kchk = reinterpret_cast<float*>(Ukn);
        for (int i = threadIdx.x; i < 4 * nsub; i += blockDim.x) kchk[i] = 0.f;
    }
    WG_TASK(P::G, nsub, g, sub);
    ZSTAMP_HEAD(0);
    const aux_t aux = aux_setup<P>(s + P::NL * P::LS, twg);
    const float2* tw = aux.tw;
    const int h = S / 2;
    const size_t cbase = (size_t)(sub * P::G + g) * P::NL * P::L;
    constexpr int RT = P::THREADS, NE = (P::NL * P::L + RT - 1) / RT;
    float2 park[NE];                                               // Pn^ (PREP: Pr^), then kn^
    for (int pass = 0; pass < (PREP ? 1 : 2); pass++) {
        const float2* qs = Q + ((size_t)pass * nsub + sub) * S * P::HP;
        for (int e = threadIdx.x; e < P::NL * P::LS; e += blockDim.x) s[e] = make_float2(0.f, 0.f);
        __syncthreads();
        ZSTAMP(0, 1 + 3 * pass);
        // the stamp's S non-zero rows, row-transformed by k_psf_rowdft: line[y] = sum_x p[y][x] W^(kx x)
        for (int e = threadIdx.x; e < P::NL * S; e += blockDim.x) {
            const int ll = e % P::NL, j = e / P::NL;
            const int kk = g * P::NL + ll;
            if (kk >= P::H) continue;
            const int y = ((j - h) % P::L + P::L) % P::L;
            s[ll * P::LS + npos(y)] = qs[(size_t)j * P::HP + kk];
        }
        __syncthreads();
        ZSTAMP(0, 2 + 3 * pass);
        fft_fwd<P>(s, tw, S - h);                                      // the stamp's rows: [0, S - h) and [L - h, L)
        ZSTAMP(0, 3 + 3 * pass);
        if (!PREP && pass == 0) {
            R_LOOP(k, e, l, p) park[k] = s[l * P::LS + npos(p)];      // Pn^ waits in registers while Pr^ is transformed
            __syncthreads();
        }
    }
    if constexpr (PREP) {
        const int t = opaque_tid();
#pragma unroll
        for (int k = 0; k < NE; k++) park[k] = ld_nt(cPr + cbase + min(t + k * RT, P::NL * P::L - 1));
    }
    const zscal z = sc[sub];
    const float sn2 = z.sn * z.sn, sr2 = z.sr * z.sr, fn2 = z.fn * z.fn, fr2 = z.fr * z.fr;
    double fs = 0.0, sk2n = 0.0, sk2r = 0.0;                      // F_S and the Parseval sums of kn^2, kr^2
    R_LOOP(k, e, l, p) {
        const int kx = g * P::NL + l;
        float2 kn = make_float2(0.f, 0.f), kr = kn;
        float4 cp = make_float4(0.f, 0.f, 0.f, 0.f);
        if (kx < P::H) {
            const double wgt = (kx == 0 || (P::L % 2 == 0 && kx == P::L / 2)) ? 1.0 : 2.0;
            const float2 pn = PREP ? s[l * P::LS + npos(p)] : park[k], pr = PREP ? park[k] : s[l * P::LS + npos(p)];
            const float pn2 = pn.x * pn.x + pn.y * pn.y, pr2 = pr.x * pr.x + pr.y * pr.y;
            const float den = (sn2 * fr2) * pr2 + (sr2 * fn2) * pn2;
            // one division per entry: 1 / den as the square of 1 / sqrt(den) (a float32 division is ~10 instructions,
            // four of them were a fifth of this kernel's arithmetic)
            const float sd = sqrtf(den), isd = 1.0f / sd, rden = isd * isd;
            cp = make_float4(pn.x, pn.y, pr.x, pr.y);
            kr = cscale(make_float2(pr.x, -pr.y), z.fr * fn2 * pn2 * rden);
            kn = cscale(make_float2(pn.x, -pn.y), z.fn * fr2 * pr2 * rden);
            fs += wgt * (double)(fn2 * pn2 * fr2 * pr2 * rden);
            sk2n += wgt * (double)(kn.x * kn.x + kn.y * kn.y);
            sk2r += wgt * (double)(kr.x * kr.x + kr.y * kr.y);
        }
        // k_img_cols gets the two spectra themselves (16 bytes per entry, one load) and forms 1 / sqrt(den) and the
        // coefficients of D^, S_n^, S_r^ from them again (rounds 3-4: A, B and sqrt(den), 20 bytes in three loads)
        if constexpr (PREP) st_nt(reinterpret_cast<float2*>(cP) + cbase + e, make_float2(cp.x, cp.y));
        else st_nt(cP + cbase + e, cp);
        if constexpr (KS) {
            constexpr int F = small_of<P>::F, M = P::L / F, HM = M / 2 + 1;
            const int ky = kofp<P>(p);
            if (kx < P::H && kx % F == 0 && ky % F == 0) {
                const size_t o = ((size_t)sub * 2 * HM + kx / F) * M + ky / F;
                Ukr[o] = kr; Ukr[o + (size_t)HM * M] = kn;
            }
        } else {
            s[l * P::LS + npos(p)] = kr;
            park[k] = kn;
        }
    }
    const bool win = !KS && 2 * wh < P::L;
    double e_all = 0.0, e_out = 0.0;
    if constexpr (!KS) {
    __syncthreads();
    ZSTAMP(0, 7);
    fft_inv<P>(s, tw);
    ZSTAMP(0, 8);
    if (win) store_u_win<P>(s, Ukr, sub, g, wh, e_all, e_out); else store_u<P>(s, Ukr, sub, g);
    __syncthreads();
    R_LOOP(k, e, l, p) s[l * P::LS + npos(p)] = park[k];
    __syncthreads();
    ZSTAMP(0, 9);
    fft_inv<P>(s, tw);
    ZSTAMP(0, 10);
    if (win) store_u_win<P>(s, Ukn, sub, g, wh, e_all, e_out); else store_u<P>(s, Ukn, sub, g);
    }
    fs = wave_sum_f64(fs); sk2n = wave_sum_f64(sk2n); sk2r = wave_sum_f64(sk2r);
    e_all = wave_sum_f64(e_all); e_out = wave_sum_f64(e_out);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = fs; red[1][threadIdx.x >> 6] = sk2n; red[2][threadIdx.x >> 6] = sk2r;
        red[3][threadIdx.x >> 6] = e_all; red[4][threadIdx.x >> 6] = e_out;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double tot = 0.0;
        for (int i = 0; i < (int)blockDim.x / 64; i++) tot += red[threadIdx.x][i];
        fs_partial[((size_t)threadIdx.x * nsub + sub) * P::G + g] = tot;      // [3][nsub][G]
    }
    if (win && (threadIdx.x == 3 || threadIdx.x == 4)) {
        // energy of k_n, k_r in this column group: all rows / the rows dropped by the window (summed over the groups
        // and checked by k_var_cols)
        double tot = 0.0;
        for (int i = 0; i < (int)blockDim.x / 64; i++) tot += red[threadIdx.x][i];
        fs_partial[((size_t)threadIdx.x * nsub + sub) * P::G + g] = tot;      // [5][nsub][G]
    }
    ZSTAMP(0, 11);
}

// bbx_zogy_refpsf_fill: pass 1 of k_psf_cols for the reference's stamps alone (Q: their row DFTs) -- the same lines, the
// same transform -- and the spectrum Pr^ of the column group into the caller's buffer in C layout (the order of R_LOOP),
// zero in the padding columns kx >= H as k_psf_cols writes them.
template <class P>
__global__ __launch_bounds__(P::THREADS, P::MINW_PSF) void k_refpsf_cols(const float2* __restrict__ Q, int S, const float2* __restrict__ twg,
                                                            float2* __restrict__ cPr, int nsub) {
    extern __shared__ float2 s[];
    WG_TASK(P::G, nsub, g, sub);
    const aux_t aux = aux_setup<P>(s + P::NL * P::LS, twg);
    const float2* tw = aux.tw;
    const int h = S / 2;
    const size_t cbase = (size_t)(sub * P::G + g) * P::NL * P::L;
    constexpr int RT = P::THREADS, NE = (P::NL * P::L + RT - 1) / RT;
    const float2* qs = Q + (size_t)sub * S * P::HP;
    for (int e = threadIdx.x; e < P::NL * P::LS; e += blockDim.x) s[e] = make_float2(0.f, 0.f);
    __syncthreads();
    for (int e = threadIdx.x; e < P::NL * S; e += blockDim.x) {
        const int ll = e % P::NL, j = e / P::NL;
        const int kk = g * P::NL + ll;
        if (kk >= P::H) continue;
        const int y = ((j - h) % P::L + P::L) % P::L;
        s[ll * P::LS + npos(y)] = qs[(size_t)j * P::HP + kk];
    }
    __syncthreads();
    fft_fwd<P>(s, tw, S - h);
    R_LOOP(k, e, l, p) cPr[cbase + e] = (g * P::NL + l < P::H) ? s[l * P::LS + npos(p)] : make_float2(0.f, 0.f);
}

// inverse row pass of kr^, kn^ -> kr, kn -> squares -> forward row pass, T tiles
template <class P>
__global__ __launch_bounds__(P::LIGHT_THREADS, P::MINW_LIGHT) void k_psf_rows(const float2* __restrict__ Ukr, const float2* __restrict__ Ukn, float inv_n2,
                                                         const float2* __restrict__ twg, float2* __restrict__ Tkr2, float2* __restrict__ Tkn2,
                                                         int nsub, int nyb, int wb, const zscal* __restrict__ sc, const double* __restrict__ fs_partial,
                                                         sub_scal* __restrict__ sub_sc, int32_t* __restrict__ d_err) {
    extern __shared__ float2 s[];
    WG_TASK(nyb, nsub, ybw, sub);
    if (ybw == 0 && threadIdx.x < 64) sub_scalars<P>(fs_partial, nsub, sub, sc[sub], nyb != P::LB, sub_sc, d_err);
    // with a row window only the blocks that hold rows < wh or >= L - wh exist: nyb = 2 wb of them
    const int yb = (nyb == P::LB || ybw < wb) ? ybw : P::LB - 2 * wb + ybw;
    ZSTAMP_HEAD(1);
    const aux_t aux = aux_setup<P>(s + P::NL * P::LS, twg);
    const float2* tw = aux.tw;
    __syncthreads();                                                // the position table is used right away
    ZSTAMP(1, 1);
    load_u_pair<P>(Ukr, Ukn, sub, yb, s, aux.pp);
    __syncthreads();
    ZSTAMP(1, 2);
    fft_inv<P>(s, tw);
    ZSTAMP(1, 3);
    C_LOOP(e, l, p) {
        float2* q = s + l * P::LS + npos(p);
        const float a = q->x * inv_n2, b = q->y * inv_n2;
        *q = make_float2(a * a, b * b);
    }
    __syncthreads();
    ZSTAMP(1, 4);
    fft_fwd<P>(s, tw);
    ZSTAMP(1, 5);
    store_t_split<P>(s, aux.pp, Tkr2, Tkn2, sub, yb);
    ZSTAMP(1, 6);
}

// ---- k_n, k_r on the small grid ------------------------------------------------------------------------------------------
// A function supported inside +-wh is given exactly by its spectrum sampled at every F-th frequency: the inverse transform of
// k^[F i][F j] on the M x M grid (M = L / F) returns k with whatever lies beyond +-M/2 folded in.  The window check therefore
// measures, per sub-image and kernel, the energy the small grid holds in the rows and columns the window drops (cells
// kchk[sub][which][all, dropped], in units of sum_x k^2 M^3; float atomics, tested by k_var_cols).
// Inverse column pass of the small half spectra K[sub][which][jx][i] -> rows Us[sub][which][y][jx] (window rows only)
template <class P, class PK>
__global__ __launch_bounds__(Z3_KS_THREADS) void k_ks_cols(const float2* __restrict__ K, const float2* __restrict__ twg, float2* __restrict__ Us,
                                                           float* __restrict__ kchk, int nsub, int wh) {
    constexpr int F = P::L / PK::L, M = PK::L, HM = PK::H, HMP = (HM + 7) / 8 * 8, NG = (HM + PK::NL - 1) / PK::NL;
    extern __shared__ float2 s[];
    __shared__ double red[2][Z3_KS_THREADS / 64];
    const int task = (int)blockIdx.x;
    if (task >= NG * 2 * nsub) return;
    const int cg = task % NG, ws = task / NG;                      // column group; (sub, which)
    float2* tws = s + PK::NL * PK::LS;
    unsigned short* pps = reinterpret_cast<unsigned short*>(tws + M);
    for (int e = threadIdx.x; e < M; e += blockDim.x) { tws[e] = twg[F * e]; pps[e] = (unsigned short)ppos<PK>(e); }
    __syncthreads();
    const float2* src = K + ((size_t)ws * HM + (size_t)cg * PK::NL) * M;
    for (int e = threadIdx.x; e < PK::NL * M; e += blockDim.x) {
        const int l = e / M, i = e - l * M;
        s[l * PK::LS + pps[i]] = (cg * PK::NL + l < HM) ? src[e] : make_float2(0.f, 0.f);
    }
    __syncthreads();
    fft_inv<PK>(s, tws);
    float2* dst = Us + (size_t)ws * M * HMP;
    double ea = 0.0, eo = 0.0;
    for (int e = threadIdx.x; e < PK::NL * M; e += blockDim.x) {
        const int y = e / PK::NL, l = e - y * PK::NL, jx = cg * PK::NL + l;
        if (jx >= HM) continue;
        const float2 v = s[l * PK::LS + npos(y)];
        const float en = ((jx == 0 || 2 * jx == M) ? 1.f : 2.f) * (v.x * v.x + v.y * v.y);      // Parseval along x
        ea += (double)en;
        if (y < wh || y >= M - wh) dst[(size_t)y * HMP + jx] = v; else eo += (double)en;
    }
    ea = wave_sum_f64(ea); eo = wave_sum_f64(eo);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = ea; red[1][threadIdx.x >> 6] = eo; }
    __syncthreads();
    if (threadIdx.x < 2) {
        double tot = 0.0;
        for (int i = 0; i < (int)blockDim.x / 64; i++) tot += red[threadIdx.x][i];
        atomicAdd(kchk + 2 * ws + threadIdx.x, (float)tot);
    }
}
// NL window rows as (k_r, k_n) pairs: inverse row pass at M -> squares, placed into lines of L points (zero outside
// [-wh, wh)) -> forward row pass at L, T tiles.  LDS: the lines and tables of side L, then NL lines and the tables of side M
template <class P, class PK>
__global__ __launch_bounds__(P::LIGHT_THREADS, P::MINW_LIGHT) void k_ks_rows(const float2* __restrict__ Us, float inv_m2, const float2* __restrict__ twg,
                                                         float2* __restrict__ Tkr2, float2* __restrict__ Tkn2, int nsub, int nyb, int wb,
                                                         const zscal* __restrict__ sc, const double* __restrict__ fs_partial,
                                                         sub_scal* __restrict__ sub_sc, int32_t* __restrict__ d_err, float* __restrict__ kchk) {
    constexpr int F = P::L / PK::L, M = PK::L, HM = PK::H, HMP = (HM + 7) / 8 * 8;
    extern __shared__ float2 s[];
    __shared__ double red[2][P::LIGHT_THREADS / 64];
    WG_TASK(nyb, nsub, ybw, sub);
    if (ybw == 0 && threadIdx.x < 64) sub_scalars<P>(fs_partial, nsub, sub, sc[sub], false, sub_sc, d_err);
    const int yb = ybw < wb ? ybw : P::LB - 2 * wb + ybw, wh = wb * P::NL;
    const aux_t aux = aux_setup<P>(s + P::NL * P::LS, twg);
    float2* ss = reinterpret_cast<float2*>(reinterpret_cast<char*>(s + P::NL * P::LS) + aux_bytes<P>());
    float2* tws = ss + P::NL * PK::LS;
    unsigned short* pps = reinterpret_cast<unsigned short*>(tws + M);
    for (int e = threadIdx.x; e < M; e += blockDim.x) { tws[e] = twg[F * e]; pps[e] = (unsigned short)ppos<PK>(e); }
    for (int e = threadIdx.x; e < P::NL * P::LS; e += blockDim.x) s[e] = make_float2(0.f, 0.f);
    for (int e = threadIdx.x; e < P::NL * PK::LS; e += blockDim.x) ss[e] = make_float2(0.f, 0.f);
    __syncthreads();
    const float2 *Ur = Us + (size_t)(2 * sub) * M * HMP, *Un = Ur + (size_t)M * HMP;
    for (int e = threadIdx.x; e < P::NL * HM; e += blockDim.x) {
        const int r = e / HM, jx = e - r * HM, y = yb * P::NL + r, ys = y < wh ? y : y - P::L + M;
        pack_store<PK>(ss + r * PK::LS, pps, jx, Ur[(size_t)ys * HMP + jx], Un[(size_t)ys * HMP + jx]);
    }
    __syncthreads();
    fft_inv<PK, P::NL>(ss, tws);
    float eor = 0.f, eon = 0.f;
    for (int e = threadIdx.x; e < P::NL * M; e += blockDim.x) {
        const int r = e / M, x = e - r * M;
        const float2 q = ss[r * PK::LS + npos(x)];
        if (x < wh || x >= M - wh) {
            const float a = q.x * inv_m2, b = q.y * inv_m2;
            s[r * P::LS + npos(x < wh ? x : x - M + P::L)] = make_float2(a * a, b * b);
        } else { eor += q.x * q.x; eon += q.y * q.y; }
    }
    __syncthreads();
    fft_fwd<P>(s, aux.tw, wh);
    store_t_split<P>(s, aux.pp, Tkr2, Tkn2, sub, yb);
    double er = wave_sum_f64((double)eor), en = wave_sum_f64((double)eon);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = er; red[1][threadIdx.x >> 6] = en; }
    __syncthreads();
    if (threadIdx.x < 2) {
        double tot = 0.0;
        for (int i = 0; i < (int)blockDim.x / 64; i++) tot += red[threadIdx.x][i];
        atomicAdd(kchk + 4 * sub + 2 * threadIdx.x + 1, (float)(tot / (double)M));      // sum_x a^2 = M sum_kx |A|^2
    }
}
template <class PK> constexpr size_t ks_tab_bytes() { return (size_t)PK::L * sizeof(float2) + (((size_t)PK::L * 2 + 15) & ~(size_t)15); }
template <class PK> constexpr size_t lds_ks_cols_bytes() { return (size_t)PK::NL * PK::LS * sizeof(float2) + ks_tab_bytes<PK>(); }

// forward column pass of one T array -> C layout
template <class P>
__global__ __launch_bounds__(P::THREADS, P::MINW_LIGHT) void k_cols_fwd(const float2* __restrict__ T, const float2* __restrict__ twg, float2* __restrict__ Cout, int nsub) {
    extern __shared__ float2 s[];
    WG_TASK(P::G, nsub, g, sub);
    const aux_t aux = aux_setup<P>(s + P::NL * P::LS, twg);
    const float2* tw = aux.tw;
    load_t_lines<P>(T, sub, g, s);
    __syncthreads();
    fft_fwd<P>(s, tw);
    const size_t cbase = (size_t)(sub * P::G + g) * P::NL * P::L;
    C_LOOP(e, l, p) Cout[cbase + e] = s[l * P::LS + npos(p)];
}

// ---- image side -------------------------------------------------------------------------------
struct frame_args {
    const float* a; const float* b;          // the two frames of a pair (new, ref)
    const float* sa; const float* sb;        // sigma images (variance pair) or NULL
    int ny, nx, size, border, nsx, vec4;
};

// cut + forward row pass of a pair of real frames: (N, R) or, with sigma images, (Vn, Vr)
template <class P>
__global__ __launch_bounds__(P::LIGHT_THREADS, P::MINW_LIGHT) void k_img_rows(frame_args f, const float2* __restrict__ twg, float2* __restrict__ Ta, float2* __restrict__ Tb, int nsub) {
    extern __shared__ float2 s[];
    WG_TASK_ROWS(P::LB, nsub, yb, sub);
    const aux_t aux = aux_setup<P>(s + P::NL * P::LS, twg);
    const float2* tw = aux.tw;
    const int y0 = yb * P::NL;
    const int sy = sub / f.nsx, sx = sub - sy * f.nsx;
    const int Y0 = sy * f.size - f.border, X0 = sx * f.size - f.border;
    if (f.vec4) {
        // groups of four pixels never straddle the frame edge (size, border, nx multiples of 4)
        constexpr int NV = P::NL * P::L / 4;
        constexpr int IL = Z3_IMG_LOADS;                        // groups of four pixels per thread and round: all of a workgroup's loads in one round trip
        for (int e0 = threadIdx.x; e0 < NV; e0 += IL * (int)blockDim.x) {
            float4 va[IL], vb[IL];
            bool in[IL];
#pragma unroll
            for (int i = 0; i < IL; i++) {
                const int e = e0 + i * (int)blockDim.x;
                va[i] = vb[i] = make_float4(0.f, 0.f, 0.f, 0.f); in[i] = false;
                if (e < NV) {
                    const int q = 4 * e, ll = q / P::L, x = q - ll * P::L;
                    const int Y = Y0 + y0 + ll, X = X0 + x;
                    if (y0 + ll < P::L && Y >= 0 && Y < f.ny && X >= 0 && X < f.nx) {
                        const size_t o = (size_t)Y * f.nx + X;
                        in[i] = true;
                        va[i] = ld_nt(reinterpret_cast<const float4*>(f.a + o)); vb[i] = ld_nt(reinterpret_cast<const float4*>(f.b + o));
                        if (f.sa) {
                            const float4 p = *reinterpret_cast<const float4*>(f.sa + o), q4 = *reinterpret_cast<const float4*>(f.sb + o);
                            va[i] = make_float4(fmaxf(va[i].x, 0.f) + p.x * p.x, fmaxf(va[i].y, 0.f) + p.y * p.y, fmaxf(va[i].z, 0.f) + p.z * p.z,
                                                fmaxf(va[i].w, 0.f) + p.w * p.w);
                            vb[i] = make_float4(fmaxf(vb[i].x, 0.f) + q4.x * q4.x, fmaxf(vb[i].y, 0.f) + q4.y * q4.y,
                                                fmaxf(vb[i].z, 0.f) + q4.z * q4.z, fmaxf(vb[i].w, 0.f) + q4.w * q4.w);
                        }
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < IL; i++) {
                const int e = e0 + i * (int)blockDim.x;
                if (e < NV) {
                    const int q = 4 * e, ll = q / P::L, x = q - ll * P::L;
                    float2* line = s + ll * P::LS;
                    line[npos(x)] = make_float2(va[i].x, vb[i].x); line[npos(x + 1)] = make_float2(va[i].y, vb[i].y);
                    line[npos(x + 2)] = make_float2(va[i].z, vb[i].z); line[npos(x + 3)] = make_float2(va[i].w, vb[i].w);
                }
            }
        }
    } else
    for (int e = threadIdx.x; e < P::NL * P::L; e += blockDim.x) {
        const int ll = e / P::L, x = e - ll * P::L;
        const int Y = Y0 + y0 + ll, X = X0 + x;
        float2 v = make_float2(0.f, 0.f);
        if (y0 + ll < P::L && Y >= 0 && Y < f.ny && X >= 0 && X < f.nx) {
            const size_t o = (size_t)Y * f.nx + X;
            v.x = f.a[o]; v.y = f.b[o];
            if (f.sa) { const float p = f.sa[o], q = f.sb[o]; v.x = fmaxf(v.x, 0.f) + p * p; v.y = fmaxf(v.y, 0.f) + q * q; }
        }
        s[ll * P::LS + npos(x)] = v;
    }
    __syncthreads();
    fft_fwd<P>(s, tw);
    store_t_split<P>(s, aux.pp, Ta, Tb, sub, yb);
}

// One frame of a pair and its variance image (frames whose groups of four pixels are aligned).  The two-for-one transforms
// pair neighbouring rows of the same image: of the NL rows of a block, lines 0 .. NL/2 - 1 carry a[2j] + i a[2j + 1], lines
// NL/2 .. NL - 1 carry V[2j] + i V[2j + 1], V = max(a, 0) + sigma^2 -- one transform of NL lines, split into the rows of
// (a^, V^) by store_t_rows.  A packed transform rounds each partner in the presence of the other; partners of the same image
// share their units, so frames, sigma maps and noise scalars times a power of two still scale S and Fpsf exactly (V is not
// a multiple of its unscaled self -- max(a, 0) grows with the factor, sigma^2 with its square -- and must not ride with a).
// The new frame goes into (T0, T2), the reference into (T1, T3): two launches of this kernel.  The reference's launch depends
// on the reference and its sigma map alone, so a caller whose reference stays the same from frame to frame runs it once
// (bbx_zogy_refrows) and bbx_zogy_frame then launches the new frame's only.
// SPL (round 5, bbx_zogy_frame_mini): the sigma image does not exist as a frame -- the kernel reads it off its mini image
// (bbx_spline.h): a table of the cubics of every frame row on every box interval (k_spl_polytable, 48 MB per map,
// mostly L2 hits here: the ~15 groups of four pixels of an interval read the same entry) instead of the frame (4N
// written, 4N x 1.125 read); a pixel costs a share of a 16-byte load and three multiply-adds.
struct frame1_args {
    const float* a; const float* sa;         // the frame; its sigma image (NULL with SPL)
    int ny, nx, size, border, nsx;
};
// sigma of the four pixels (Y, X .. X + 3) of one patch off the cubic table (patch widths, X multiples of 4): interval and
// remainder of the first, steps for the others; the group lies in one interval or in two neighbouring ones: both cubics are loaded
__device__ __forceinline__ float4 spl_sigma4(const bbx_spl& sp, int Y, int X) {
    int c, r;
    bbx_spl_axis(X, sp.pw, sp.rpw, sp.px, sp.npad, sp.nx1, sp.dx, sp.rdx, c, r);
    const float4* t = sp.poly + (size_t)Y * sp.cnx + c;
    const int step = (r + 3 * sp.nx1 >= sp.dx) ? 1 : 0;
    const float4 p0 = t[0], p1 = t[step];
    float sg[4];
    bool w = false;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        sg[k] = bbx_spl_horner(w ? p1 : p0, (float)r * sp.rdx);
        r += sp.nx1; if (r >= sp.dx) { r -= sp.dx; w = true; }
    }
    return make_float4(sg[0], sg[1], sg[2], sg[3]);
}
__device__ __forceinline__ float4 var4(float4 v, float4 p) {
    return make_float4(fmaxf(v.x, 0.f) + p.x * p.x, fmaxf(v.y, 0.f) + p.y * p.y, fmaxf(v.z, 0.f) + p.z * p.z, fmaxf(v.w, 0.f) + p.w * p.w);
}
// Hermitian split of the packed row pairs (LDS, spectrum order) -> the rows of two half spectra, T tiles of row block yb:
// line j holds rows 2j, 2j + 1 of Ta, line NL/2 + j those of Tb
template <class P> __device__ __forceinline__ void store_t_rows(const float2* s, const unsigned short* pp, float2* __restrict__ Ta, float2* __restrict__ Tb, int sub,
                                                                 int yb) {
    const size_t base = (size_t)sub * P::UNIT + (size_t)yb * P::HP * P::NL;
    for (int kx = threadIdx.x; kx < P::H; kx += blockDim.x) {
        const int pk = pp[kx], pm = pp[kx ? P::L - kx : 0];
        float4* ta = reinterpret_cast<float4*>(Ta + base + (size_t)kx * P::NL);
        float4* tb = reinterpret_cast<float4*>(Tb + base + (size_t)kx * P::NL);
#pragma unroll
        for (int j = 0; j < P::NL / 2; j++) {
            const float2 ak = s[j * P::LS + pk], am = s[j * P::LS + pm], bk = s[(P::NL / 2 + j) * P::LS + pk], bm = s[(P::NL / 2 + j) * P::LS + pm];
            st_nt(ta + j, make_float4(0.5f * (ak.x + am.x), 0.5f * (ak.y - am.y), 0.5f * (ak.y + am.y), 0.5f * (am.x - ak.x)));
            st_nt(tb + j, make_float4(0.5f * (bk.x + bm.x), 0.5f * (bk.y - bm.y), 0.5f * (bk.y + bm.y), 0.5f * (bm.x - bk.x)));
        }
    }
}
template <class P, bool SPL>
__global__ __launch_bounds__(P::LIGHT_THREADS, P::MINW_LIGHT) void k_img_rows_one(frame1_args f, const float2* __restrict__ twg, float2* __restrict__ Ta,
                                                                               float2* __restrict__ Tva, int nsub, bbx_spl sp) {
    extern __shared__ float2 s[];
    WG_TASK_ROWS(P::LB, nsub, yb, sub);
    ZSTAMP_HEAD(2);
    const aux_t aux = aux_setup<P>(s + P::NL * P::LS, twg);
    const float2* tw = aux.tw;
    const int y0 = yb * P::NL;
    const int sy = sub / f.nsx, sx = sub - sy * f.nsx;
    const int Y0 = sy * f.size - f.border, X0 = sx * f.size - f.border;
    // an item: the same group of four pixels of the two rows of a pair
    constexpr int XG = P::L / 4, NI = (P::NL / 2) * XG, NP = (NI + P::LIGHT_THREADS - 1) / P::LIGHT_THREADS;
    {
        float4 va[NP][2], pa[NP][2];
#pragma unroll
        for (int i = 0; i < NP; i++) {
            const int e = (int)threadIdx.x + i * P::LIGHT_THREADS;
#pragma unroll
            for (int h = 0; h < 2; h++) {
                va[i][h] = pa[i][h] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (e < NI) {
                    const int j = e / XG, x = 4 * (e - j * XG), ll = 2 * j + h;
                    const int Y = Y0 + y0 + ll, X = X0 + x;
                    if (y0 + ll < P::L && Y >= 0 && Y < f.ny && X >= 0 && X < f.nx) {
                        const size_t o = (size_t)Y * f.nx + X;
                        va[i][h] = ld_nt(reinterpret_cast<const float4*>(f.a + o));
                        if (!SPL) pa[i][h] = ld_nt(reinterpret_cast<const float4*>(f.sa + o));
                    }
                }
            }
        }
        if (SPL) {
#pragma unroll
            for (int i = 0; i < NP; i++) {
                const int e = (int)threadIdx.x + i * P::LIGHT_THREADS;
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    if (e < NI) {
                        const int j = e / XG, x = 4 * (e - j * XG), ll = 2 * j + h;
                        const int Y = Y0 + y0 + ll, X = X0 + x;
                        if (y0 + ll < P::L && Y >= 0 && Y < f.ny && X >= 0 && X < f.nx) pa[i][h] = spl_sigma4(sp, Y, X);
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NP; i++) {
            const int e = (int)threadIdx.x + i * P::LIGHT_THREADS;
            if (e < NI) {
                const int j = e / XG, x = 4 * (e - j * XG);
                float2 *la = s + j * P::LS, *lv = s + (P::NL / 2 + j) * P::LS;
                const float4 a0 = va[i][0], a1 = va[i][1], v0 = var4(a0, pa[i][0]), v1 = var4(a1, pa[i][1]);
                la[npos(x)] = make_float2(a0.x, a1.x); la[npos(x + 1)] = make_float2(a0.y, a1.y);
                la[npos(x + 2)] = make_float2(a0.z, a1.z); la[npos(x + 3)] = make_float2(a0.w, a1.w);
                lv[npos(x)] = make_float2(v0.x, v1.x); lv[npos(x + 1)] = make_float2(v0.y, v1.y);
                lv[npos(x + 2)] = make_float2(v0.z, v1.z); lv[npos(x + 3)] = make_float2(v0.w, v1.w);
            }
        }
    }
    __syncthreads();
    ZSTAMP(2, 1);
    fft_fwd<P>(s, tw);
    ZSTAMP(2, 2);
    store_t_rows<P>(s, aux.pp, Ta, Tva, sub, yb);
    ZSTAMP(2, 3);
}

// column pass of the image pair: D^ = A N^ - B R^, Sn^ = kn^ N^, Sr^ = kr^ R^ and back (U tiles)
// PREP (prepared reference, bbx_zogy_refrows): TR is R^ itself, column-transformed by k_cols_fwd (C layout, the order of
// R_LOOP): a thread loads its own entries into registers behind the transform of N, N^ stays in the lines, and the load of
// the T_R tiles, its two barriers and one forward transform are gone.
// PPSF 1 (prepared reference PSF as well, bbx_zogy_refpsf): cP is a float2 array of Pn^ alone and cPr the prepared Pr^; the
// float4 of an entry is put together from two 8-byte loads, in the same two batches.
// PPSF 2 (the same on the small-grid path): no Pn^ array and no k_psf_cols launch either.  The workgroup first does pass 1 of
// k_psf_cols for the new stamps (pf.Q: their row DFTs), N's tiles and its Pr^ entries travelling to registers behind that
// transform; a loop of its own, in front of N's transform, parks Pn^ and emits what k_psf_cols<P, true> emitted, by the same
// expressions in the same thread-to-entry mapping: the F_S / Parseval partial sums, the samples of k_r^, k_n^ for the small
// grid (pf.Ksm) and the zeroed cells of the window check (pf.kchk).  Of Pr^ the first half stays in registers across N's
// transform; the second is read again behind it (all of Pn^, Pr^ and R^ parked at once do not fit 85 VGPRs).
struct psf_fuse_args { const float2* Q; int S; float* kchk; float2* Ksm; double* fs_partial; };
template <class P, bool PREP, int PPSF = 0>
__global__ __launch_bounds__(P::THREADS, P::MINW) void k_img_cols(const float2* __restrict__ TN, const float2* __restrict__ TR, const float4* __restrict__ cP,
                                                         const float2* __restrict__ cPr, const zscal* __restrict__ sc, const float2* __restrict__ twg,
                                                         float2* __restrict__ UD, float2* __restrict__ USn, float2* __restrict__ USr,
                                                         float2* __restrict__ HSn, float2* __restrict__ HSr, int nsub, chunk_args ch, psf_fuse_args pf) {
    extern __shared__ float2 s[];
    if (PPSF == 2 && blockIdx.x == 0) {
        for (int i = threadIdx.x; i < 4 * nsub; i += blockDim.x) pf.kchk[i] = 0.f;
    }
    WG_TASK(P::G, nsub, g, sub);
    ZSTAMP_HEAD(3);
    const aux_t aux = aux_setup<P>(s + P::NL * P::LS, twg);
    const float2* tw = aux.tw;
    const size_t cbase = (size_t)(sub * P::G + g) * P::NL * P::L;
    constexpr int RT = P::THREADS, NE = (P::NL * P::L + RT - 1) / RT;
    constexpr int NC0 = NE / 2;
    float4 c0[NC0], c1[NE - NC0];
    float2 pnr[PPSF == 2 ? NE : 1];                                // PPSF 2: this thread's entries of Pn^
    if constexpr (PPSF == 2) {
        const int h = pf.S / 2;
        const float2* qs = pf.Q + (size_t)sub * pf.S * P::HP;
        for (int e = threadIdx.x; e < P::NL * P::LS; e += blockDim.x) s[e] = make_float2(0.f, 0.f);
        __syncthreads();
        for (int e = threadIdx.x; e < P::NL * pf.S; e += blockDim.x) {
            const int ll = e % P::NL, j = e / P::NL;
            const int kk = g * P::NL + ll;
            if (kk >= P::H) continue;
            const int y = ((j - h) % P::L + P::L) % P::L;
            s[ll * P::LS + npos(y)] = qs[(size_t)j * P::HP + kk];
        }
        __syncthreads();
        t_regs<P, P::THREADS> rn;                                  // T_N and Pr^ on their way while the stamps are transformed
        fetch_t_lines<P, P::THREADS>(TN, sub, g, rn);
        float2 pra[NE];
        {
            // (the second half is read again behind N's transform, as the batches below have it: plain loads keep it near)
            const int t = opaque_tid();
#pragma unroll
            for (int k = 0; k < NE; k++) {
                const float2* q = cPr + cbase + min(t + k * RT, P::NL * P::L - 1);
                pra[k] = k < NC0 ? ld_nt(q) : *q;
            }
        }
        fft_fwd<P>(s, tw, pf.S - h);
        // what k_psf_cols<P, true> computes from the two spectra, by its expressions in its thread-to-entry mapping (its own
        // 1 / den: the square of 1 / sqrt(den) by division); Pn^ is parked, zero in the padding columns kx >= H as k_psf_cols
        // writes them
        const zscal z = sc[sub];
        const float sn2 = z.sn * z.sn, sr2 = z.sr * z.sr, fn2 = z.fn * z.fn, fr2 = z.fr * z.fr;
        double fs = 0.0, sk2n = 0.0, sk2r = 0.0;
        R_LOOP(k, e, l, p) {
            const int kx = g * P::NL + l;
            float2 pn = make_float2(0.f, 0.f);
            if (kx < P::H) {
                const double wgt = (kx == 0 || (P::L % 2 == 0 && kx == P::L / 2)) ? 1.0 : 2.0;
                const float2 pr = pra[k];
                pn = s[l * P::LS + npos(p)];
                const float pn2 = pn.x * pn.x + pn.y * pn.y, pr2 = pr.x * pr.x + pr.y * pr.y;
                const float den = (sn2 * fr2) * pr2 + (sr2 * fn2) * pn2;
                const float sd = sqrtf(den), isd = 1.0f / sd, rden = isd * isd;
                const float2 kr = cscale(make_float2(pr.x, -pr.y), z.fr * fn2 * pn2 * rden);
                const float2 kn = cscale(make_float2(pn.x, -pn.y), z.fn * fr2 * pr2 * rden);
                fs += wgt * (double)(fn2 * pn2 * fr2 * pr2 * rden);
                sk2n += wgt * (double)(kn.x * kn.x + kn.y * kn.y);
                sk2r += wgt * (double)(kr.x * kr.x + kr.y * kr.y);
                constexpr int F = small_of<P>::F, M = P::L / F, HM = M / 2 + 1;
                const int ky = kofp<P>(p);
                if (kx % F == 0 && ky % F == 0) {
                    const size_t o = ((size_t)sub * 2 * HM + kx / F) * M + ky / F;
                    pf.Ksm[o] = kr; pf.Ksm[o + (size_t)HM * M] = kn;
                }
            }
            pnr[k] = pn;
        }
#pragma unroll
        for (int k = 0; k < NC0; k++) c0[k] = make_float4(0.f, 0.f, pra[k].x, pra[k].y);
        // the partial sums of the column group, reduced as k_psf_cols reduces them
        __shared__ double red[3][P::THREADS / 64];
        fs = wave_sum_f64(fs); sk2n = wave_sum_f64(sk2n); sk2r = wave_sum_f64(sk2r);
        if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = fs; red[1][threadIdx.x >> 6] = sk2n; red[2][threadIdx.x >> 6] = sk2r; }
        __syncthreads();
        if (threadIdx.x < 3) {
            double tot = 0.0;
            for (int i = 0; i < (int)blockDim.x / 64; i++) tot += red[threadIdx.x][i];
            pf.fs_partial[((size_t)threadIdx.x * nsub + sub) * P::G + g] = tot;      // [3][nsub][G]
        }
        pack_t_lines<P, P::THREADS>(rn, s);
    } else
    load_t_lines<P>(TN, sub, g, s);
    // N^ waits in registers for R^; then one loop makes D^, S_n^ (both parked) and S_r^ (into the lines) from A, B, sqrt(den)
    float2 park[NE], parkd[NE];
    // the PSF spectra of this column group: the first half of a thread's entries is on its way while R is transformed, the
    // second half goes out in one round behind it (a load inside the guarded loop below waits for its own round trip in
    // every iteration: 8 x 2 700 cycles of this kernel's 95 000 in round 4)
    float2 rh[PREP ? NE : 1];                                      // PREP: this thread's entries of R^
    static_assert(PREP || !PPSF, "prepared PSF spectra go with prepared rows");
    static_assert(PPSF != 2 || small_of<P>::ok, "Pn^ is formed here on the small-grid path only");
    const auto ld_c = [&](int e) -> float4 {
        if constexpr (PPSF == 2) {
            const float2 pr = ld_nt(cPr + cbase + e);              // (x, y stay unused: Pn^ is in pnr)
            return make_float4(0.f, 0.f, pr.x, pr.y);
        } else if constexpr (PPSF == 1) {
            const float2 pn = ld_nt(reinterpret_cast<const float2*>(cP) + cbase + e), pr = ld_nt(cPr + cbase + e);
            return make_float4(pn.x, pn.y, pr.x, pr.y);
        } else return ld_nt(cP + cbase + e);
    };
    if constexpr (PREP) {
        {
            const int t = opaque_tid();
#pragma unroll
            for (int k = 0; k < NE; k++) rh[k] = ld_nt(TR + cbase + min(t + k * RT, P::NL * P::L - 1));
#pragma unroll
            for (int k = 0; k < NC0; k++) if (PPSF != 2) c0[k] = ld_c(min(t + k * RT, P::NL * P::L - 1));
        }
        __syncthreads();
        ZSTAMP(3, 1);
        fft_fwd<P>(s, tw);
        ZSTAMP(3, 4);
    } else {
#ifndef Z3_NO_PREFETCH
    t_regs<P, P::THREADS> rr;                                      // T_R on its way while T_N is transformed
    fetch_t_lines<P, P::THREADS>(TR, sub, g, rr);
#endif
    __syncthreads();
    ZSTAMP(3, 1);
    fft_fwd<P>(s, tw);
    ZSTAMP(3, 2);
    R_LOOP(k, e, l, p) park[k] = s[l * P::LS + npos(p)];
    __syncthreads();
#ifndef Z3_NO_PREFETCH
    pack_t_lines<P, P::THREADS>(rr, s);
#else
    load_t_lines<P>(TR, sub, g, s);
#endif
    __syncthreads();
    ZSTAMP(3, 3);
    {
        const int t = opaque_tid();
#pragma unroll
        for (int k = 0; k < NC0; k++) c0[k] = ld_nt(cP + cbase + min(t + k * RT, P::NL * P::L - 1));
    }
    fft_fwd<P>(s, tw);
    ZSTAMP(3, 4);
    }
    {
        const int t = opaque_tid();
#pragma unroll
        for (int k = NC0; k < NE; k++) c1[k - NC0] = ld_c(min(t + k * RT, P::NL * P::L - 1));
    }
    const zscal z = sc[sub];
    const float cn = (z.sr * z.sr) * (z.fn * z.fn), cr = (z.sn * z.sn) * (z.fr * z.fr);      // den = cr |Pr^|^2 + cn |Pn^|^2
    const float kfn = z.fn * (z.fr * z.fr), kfr = z.fr * (z.fn * z.fn);
    R_LOOP(k, e, l, p) {
        float2* q = s + l * P::LS + npos(p);
        const float2 r = PREP ? rh[PREP ? k : 0] : *q, n = PREP ? *q : park[k];
        const float4 c = k < NC0 ? c0[k < NC0 ? k : 0] : c1[k >= NC0 ? k - NC0 : 0];      // (Pn^, Pr^); zero in the padding columns kx >= H
        const float2 pn = PPSF == 2 ? pnr[PPSF == 2 ? k : 0] : make_float2(c.x, c.y), pr = make_float2(c.z, c.w);
        const float pn2 = pn.x * pn.x + pn.y * pn.y, pr2 = pr.x * pr.x + pr.y * pr.y;
        const float den = cr * pr2 + cn * pn2;
        const float isd = (g * P::NL + l < P::H) ? __builtin_amdgcn_rsqf(den) : 0.f, rden = isd * isd;
        // D^ = (f_r Pr^ N^ - f_n Pn^ R^) / sqrt(den), S_n^ = k_n^ N^, S_r^ = k_r^ R^ with k_n^ = f_n f_r^2 conj(Pn^) |Pr^|^2 / den
        const float2 an = cmul(pr, n), br = cmul(pn, r);
        const float da = z.fr * isd, db = z.fn * isd;
        parkd[k] = make_float2(an.x * da - br.x * db, an.y * da - br.y * db);
        park[k] = cscale(cmulc(n, pn), kfn * pr2 * rden);           // conj(Pn^) n
        *q = cscale(cmulc(r, pr), kfr * pn2 * rden);
    }
    __syncthreads();
    ZSTAMP(3, 5);
    fft_inv<P>(s, tw);
    ZSTAMP(3, 6);
    store_u<P>(s, USr, sub, g, HSr, ch);
    __syncthreads();
    R_LOOP(k, e, l, p) s[l * P::LS + npos(p)] = park[k];
    __syncthreads();
    ZSTAMP(3, 7);
    fft_inv<P>(s, tw);
    ZSTAMP(3, 8);
    store_u<P>(s, USn, sub, g, HSn, ch);
    __syncthreads();
    R_LOOP(k, e, l, p) s[l * P::LS + npos(p)] = parkd[k];
    __syncthreads();
    ZSTAMP(3, 9);
    fft_inv<P>(s, tw);
    ZSTAMP(3, 10);
    store_u<P>(s, UD, sub, g);
    ZSTAMP(3, 11);
}

// column pass of the variance pair: V(S)^ = Vn^ (kn^2)^ + Vr^ (kr^2)^ and back (U tiles).  The spectra (kn^2)^, (kr^2)^
// get their column pass here as well (their row pass is k_psf_rows): a workgroup needs exactly its own column group
// of them, so they go from the T tiles through the transform into registers and never to HBM as coefficient arrays.
// PREP (prepared reference): TVr is Vr^ itself (C layout, k_cols_fwd): loaded into registers behind the transform of k_r^2,
// whose spectrum then stays in the lines -- no T_Vr tiles, no fourth forward transform.
template <class P, bool PREP>
__global__ __launch_bounds__(P::VAR_THREADS, P::VAR_MINW) void k_var_cols(const float2* __restrict__ TVn, const float2* __restrict__ TVr, const float2* __restrict__ Tk2n,
                                                         const float2* __restrict__ Tk2r, const float2* __restrict__ twg,
                                                         float2* __restrict__ UVS, const sub_scal* __restrict__ sub_sc, int nsub, int wh,
                                                         int32_t* __restrict__ ticket, const float* __restrict__ kchk, int32_t* __restrict__ d_err) {
    extern __shared__ float2 s[];
    if (blockIdx.x == 0 && threadIdx.x == 0) *ticket = 0;          // the final kernel's chunk counter (next launch on this stream)
    if (kchk && blockIdx.x == 0) {
        // small-grid path: what k_n, k_r of a sub-image hold in the rows and columns the window drops (k_ks_cols, k_ks_rows)
        for (int i = threadIdx.x; i < 2 * nsub; i += blockDim.x)
            if (!(kchk[2 * i + 1] <= (float)Z3_KWIN_TOL * kchk[2 * i])) atomicOr(d_err, BBX_DERR_PSF_WINDOW);
    }
    WG_TASK(P::G, nsub, g, sub);
    ZSTAMP_HEAD(4);
    const aux_t aux = aux_setup<P>(s + P::NL * P::LS, twg);
    const float2* tw = aux.tw;
    constexpr int RT = P::VAR_THREADS, NE = (P::NL * P::L + RT - 1) / RT;        // two parked arrays: 512 threads, <= 128 VGPRs, no spills
    float2 park[NE], coef[NE];
    const bool win = 2 * wh < P::L;
    if (win) load_t_lines_win<P>(Tk2n, sub, g, s, wh); else load_t_lines<P>(Tk2n, sub, g, s);
    t_regs<P, P::VAR_THREADS> rr;                                  // Vn^ (then Vr^) on its way while the k^2 spectrum is transformed
    fetch_t_lines<P, P::VAR_THREADS>(TVn, sub, g, rr);
    __syncthreads();
    ZSTAMP(4, 1);
    fft_fwd<P>(s, tw, win ? wh : 0);
    ZSTAMP(4, 2);
#if defined(Z3_STAMPS) && defined(Z3_FFT2X)          // diagnostic: the same transform once more (results wrong, timing only)
    fft_fwd<P>(s, tw, win ? wh : 0);
    ZSTAMP(4, 12);
    fft_fwd<P>(s, tw, win ? wh : 0);
    ZSTAMP(4, 13);
#endif
    R_LOOP(k, e, l, p) coef[k] = s[l * P::LS + npos(p)];                       // (kn^2)^
    __syncthreads();
    pack_t_lines<P, P::VAR_THREADS>(rr, s);
    __syncthreads();
    ZSTAMP(4, 3);
    fft_fwd<P>(s, tw);
    ZSTAMP(4, 4);
    R_LOOP(k, e, l, p) park[k] = cmul(coef[k], s[l * P::LS + npos(p)]);
    __syncthreads();
    if (win) load_t_lines_win<P>(Tk2r, sub, g, s, wh); else load_t_lines<P>(Tk2r, sub, g, s);
    if constexpr (PREP) {
        const size_t cbase = (size_t)(sub * P::G + g) * P::NL * P::L;
        const int t = opaque_tid();
#pragma unroll
        for (int k = 0; k < NE; k++) coef[k] = ld_nt(TVr + cbase + min(t + k * RT, P::NL * P::L - 1));      // Vr^
        __syncthreads();
        ZSTAMP(4, 5);
        fft_fwd<P>(s, tw, win ? wh : 0);
        ZSTAMP(4, 8);
    } else {
    constexpr int NH = t_regs<P, P::VAR_THREADS>::N / 4;          // (more of it beside the parked product: spills)
    fetch_t_lines<P, P::VAR_THREADS, 0, NH>(TVr, sub, g, rr);
    __syncthreads();
    ZSTAMP(4, 5);
    fft_fwd<P>(s, tw, win ? wh : 0);
    ZSTAMP(4, 6);
    R_LOOP(k, e, l, p) coef[k] = s[l * P::LS + npos(p)];                       // (kr^2)^
    __syncthreads();
    fetch_t_lines<P, P::VAR_THREADS, NH>(TVr, sub, g, rr);
    pack_t_lines<P, P::VAR_THREADS>(rr, s);
    __syncthreads();
    ZSTAMP(4, 7);
    fft_fwd<P>(s, tw);
    ZSTAMP(4, 8);
    }
    const float beta = sub_sc[sub].beta;
    R_LOOP(k, e, l, p) {
        float2* q = s + l * P::LS + npos(p);
        const float2 v = PREP ? cmul(*q, coef[k]) : cmul(coef[k], *q);          // (kr^2)^ Vr^, the factors in the same order
        *q = make_float2((park[k].x + v.x) * beta, (park[k].y + v.y) * beta);
    }
    __syncthreads();
    ZSTAMP(4, 9);
    fft_inv<P>(s, tw);
    ZSTAMP(4, 10);
    store_u<P>(s, UVS, sub, g);
    ZSTAMP(4, 11);
}

struct out_args {
    float* D; float* S; float* Scorr; float* Fpsf; float* Fpsferr;      // full frames [ny][nx]; S may be NULL
    int ny, nx, size, border, nsx, vec4;
};

// inverse row pass of (D, V_S) and (Sn, Sr) + the final algebra, written into the full frames.  A workgroup takes a chunk of
// consecutive blocks of NL rows of one sub-image (round 5; one block per workgroup before): the tables are set up once, the
// tiles of the next block are on their way while this one is transformed (registers), and the row above a block -- needed
// for the finite differences of V_ast -- is the last row of the block before it, kept in LDS: only a chunk's first block
// transforms a fifth line, taken from the halo arrays.
template <class P>
__global__ __launch_bounds__(P::FIN_THREADS, P::FIN_MINW) void k_final_rows(const float2* __restrict__ UD, const float2* __restrict__ UVS,
                                                           const float2* __restrict__ USn, const float2* __restrict__ USr,
                                                           const float2* __restrict__ HSn, const float2* __restrict__ HSr,
                                                           const zscal* __restrict__ sc, const sub_scal* __restrict__ sub_sc,
                                                           float inv_n2, const float2* __restrict__ twg, out_args o, chunk_args ch,
                                                           const int2* __restrict__ tasks, int ntasks, int32_t* __restrict__ ticket,
                                                           int nsub, float cand_thr, uint32_t* __restrict__ cand_list,
                                                           int32_t* __restrict__ cand_cnt, uint32_t cand_cap, int32_t* __restrict__ d_err) {
    extern __shared__ float2 s[];
    float2* hline = s + P::NL * P::LS;                              // the row above the block
    __shared__ int s_task;
    ZSTAMP_HEAD(5);
    const aux_t aux = aux_setup<P>(s + (P::NL + 1) * P::LS, twg);
    const float2* tw = aux.tw;
    // chunks are handed out by a ticket counter (zeroed by k_var_cols), longest first: the workgroups of a CU do not run at
    // the same speed (the older one wins the issue slots), a fixed share per workgroup left the slow ones 15 % behind
    for (;;) {
    __syncthreads();                                                // the chunk before is done with the lines and s_task
    if (threadIdx.x == 0) s_task = atomicAdd(ticket, 1);
    __syncthreads();
    const int task_ = __builtin_amdgcn_readfirstlane(s_task);      // wave-uniform: what follows from it lives in scalar registers
    if (task_ >= ntasks) break;
    const int sub = tasks[task_].x, cc = tasks[task_].y;
    const int ybA = chunk_start(ch, cc), ybB = chunk_start(ch, cc + 1);
    const zscal z = sc[sub];
    const sub_scal ss = sub_sc[sub];
    const float sn2 = z.sn * z.sn, sr2 = z.sr * z.sr, fn2 = z.fn * z.fn, fr2 = z.fr * z.fr;
    const float fD = z.fr * z.fn / sqrtf(sn2 * fr2 + sr2 * fn2);
    const float dx2 = z.dx * z.dx, dy2 = z.dy * z.dy;
    const int sy = sub / o.nsx, sx = sub - sy * o.nsx;
    constexpr int KX = (P::L + P::FIN_THREADS - 1) / P::FIN_THREADS;   // pixels of a row per thread: x = border + t + k T
    // the chunk's first block: both pairs and the row above it go out now
    u_regs<P, P::FIN_THREADS> ra, rb;
    fetch_u_pair<P, P::FIN_THREADS>(UD, UVS, sub, ybA, ra);
    fetch_u_pair<P, P::FIN_THREADS>(USn, USr, sub, ybA, rb);
    static_assert(P::H <= 2 * P::FIN_THREADS, "halo line: two entries per thread");
    float2 ha[2], hb[2];
    {
        const size_t hbase = ((size_t)sub * ch.nch + cc) * P::HP;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int kx = (int)threadIdx.x + i * P::FIN_THREADS;
            if (kx < P::H) { ha[i] = HSn[hbase + kx]; hb[i] = HSr[hbase + kx]; }
        }
    }
    __syncthreads();                                                // tables and scalars
    ZSTAMP(5, 1);
    // the row above the chunk (spectrum order) waits in the fifth line: the first (D, V_S) transform leaves it alone
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int kx = (int)threadIdx.x + i * P::FIN_THREADS;
        if (kx < P::H) pack_store<P>(hline, aux.pp, kx, ha[i], hb[i]);
    }
    const float ifs = 1.0f / ss.fs, ifD = inv_n2 / fD, vscale = inv_n2 * ss.ibeta;
    for (int yb = ybA; yb < ybB; yb++) {
        const int y0 = yb * P::NL;
        const bool first = yb == ybA, more = yb + 1 < ybB;
        // (D, V_S): D goes out at once, V_S waits in registers (the same thread takes the same pixels below)
        float vsr[P::NL][KX];
        // (the thread index goes through an empty asm in every phase: the offsets of each phase are worked out again instead of
        // living in registers across the whole loop -- with them the kernel spills)
        pack_u_pair<P, P::FIN_THREADS>(ra, yb, s, aux.pp, opaque_tid());
        __syncthreads();
        fft_inv<P>(s, tw);
        if (more) fetch_u_pair<P, P::FIN_THREADS>(UD, UVS, sub, yb + 1, ra, opaque_tid());         // on its way behind the rest of this block
        const int td = opaque_tid();
#pragma unroll
        for (int l = 0; l < P::NL; l++) {
            const int y = y0 + l, Y = sy * o.size + (y - o.border);
            const bool rowok = y >= o.border && y < o.border + o.size && Y < o.ny;
#pragma unroll
            for (int k = 0; k < KX; k++) {
                const int xi = td + k * P::FIN_THREADS, Xf = sx * o.size + xi;
                vsr[l][k] = 0.f;
                if (xi < o.size) {
                    const float2 v = s[l * P::LS + npos(o.border + xi)];
                    vsr[l][k] = v.y * vscale;
                    if (rowok && Xf < o.nx) st_nt(o.D + (size_t)Y * o.nx + Xf, v.x * ifD);
                }
            }
        }
        __syncthreads();
        // (Sn, Sr): the block's rows; the row above them is in hline already (real space) unless this is the chunk's first block
        pack_u_pair<P, P::FIN_THREADS>(rb, yb, s, aux.pp, opaque_tid());
        __syncthreads();
        if (first) fft_inv<P, P::NL + 1>(s, tw); else fft_inv<P>(s, tw);
        if (more) fetch_u_pair<P, P::FIN_THREADS>(USn, USr, sub, yb + 1, rb, opaque_tid());
        const int tf = opaque_tid();
#pragma unroll
        for (int l = 0; l < P::NL; l++) {
            const int y = y0 + l, Y = sy * o.size + (y - o.border);
            if (!(y >= o.border && y < o.border + o.size && Y < o.ny)) continue;
            const float2* line = s + l * P::LS;
            const float2* upline = l ? line - P::LS : hline;
#pragma unroll
            for (int k = 0; k < KX; k++) {
                const int xi = tf + k * P::FIN_THREADS, Xf = sx * o.size + xi, xx = o.border + xi;
                if (xi >= o.size || Xf >= o.nx) continue;
                const float2 c = cscale(line[npos(xx)], inv_n2);                              // (Sn, Sr) here
                const float2 up = cscale(upline[npos(xx)], inv_n2), lf = cscale(line[npos(xx == 0 ? P::L - 1 : xx - 1)], inv_n2);
                const float sval = c.x - c.y;                                                  // S = Sn - Sr
                const float dSndy = c.x - up.x, dSndx = c.x - lf.x, dSrdy = c.y - up.y, dSrdx = c.y - lf.y;
                const float vast = dx2 * (dSndx * dSndx + dSrdx * dSrdx) + dy2 * (dSndy * dSndy + dSrdy * dSrdy);
                const float vs = vsr[l][k];
                const size_t q = (size_t)Y * o.nx + Xf;
                if (o.S) st_nt(o.S + q, sval);
#ifndef Z3_EXACT_SQRT
                // v_rsq_f32 / v_sqrt_f32 (1 ulp) instead of the correctly rounded division and square roots (~30 instructions per
                // pixel: 8 % of this kernel); the transforms in front are good to ~1e-6 of the image scale
                const float scv = sval * __builtin_amdgcn_rsqf(vs + vast);
                st_nt(o.Scorr + q, scv);
                st_nt(o.Fpsf + q, sval * ifs);
                st_nt(o.Fpsferr + q, __builtin_amdgcn_sqrtf(fmaxf(vs, 0.f)) * ifs);
#else
                const float scv = sval / sqrtf(vs + vast);
                o.Scorr[q] = scv;
                o.Fpsf[q] = sval * ifs;
                o.Fpsferr[q] = sqrtf(fmaxf(vs, 0.f)) * ifs;
#endif
                // transient candidates (bbx_zogy_candidates): the pixels bbx_find_peaks would collect in a pass of its own over
                // the Scorr frame.  They are rare (a few thousand per frame): one reservation per wave that holds any.
                if (cand_thr > 0.f) {
                    const bool hit = fabsf(scv) >= cand_thr;             // NaN compares false
                    const unsigned long long hm = __builtin_amdgcn_ballot_w64(hit);
                    if (hm) {
                        const int leader = (int)__builtin_ctzll(hm);
                        unsigned base = 0;
                        if ((tf & 63) == leader) base = atomicAdd((unsigned*)cand_cnt, (unsigned)__popcll(hm));
                        base = (unsigned)__builtin_amdgcn_readlane((int)base, leader);
                        if (hit) {
                            const unsigned k2 = base + __builtin_amdgcn_mbcnt_hi((unsigned)(hm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)hm, 0u));
                            if (k2 < cand_cap) cand_list[k2] = (uint32_t)q; else atomicOr(d_err, BBX_DERR_LIST_OVERFLOW);
                        }
                    }
                }
            }
        }
        if (more) {
            // the block's last row is the row above the next block
            __syncthreads();
            const float2* last = s + (P::NL - 1) * P::LS;
            for (int e = opaque_tid(); e < P::LP; e += P::FIN_THREADS) hline[e] = last[e];
            __syncthreads();
        }
    }
    }
    ZSTAMP(5, 8);
}

// ---- host side --------------------------------------------------------------------------------
// The one list of sub-image sides and their plans: f is called with a value of the side's Plan type, and its result
// returned; a side without a plan gives [none].
template <class R, class F> static inline R with_plan(int L, R none, F&& f) {
    switch (L) {
        case 1400: return f(Plan<Z3_PLAN1400>{});
        case 140: return f(Plan<5, 7, 4>{});
        case 128: return f(Plan<8, 16>{});
        case 100: return f(Plan<5, 5, 4>{});
        case 64: return f(Plan<8, 8>{});
    }
    return none;
}

// Chunks of the final kernel: every sub-image's nyb row blocks are cut the same way into runs of decreasing length (guided
// schedule: a round of nslots / nsub chunks per sub-image takes two thirds of what is left, down to 2 blocks), and the tasks
// (sub-image, chunk) are listed longest first: the first round fills every workgroup slot, the short ones at the end even
// out the workgroups' different speeds.  Built once per geometry, kept with the context's twiddle table.
struct zogy_chunk_plan { int key[4]; int nch, ntasks; int* d_start; int2* d_tasks; };
static int chunk_plan(bbx_ctx* ctx, zogy_chunk_plan* pl, int yb0, int nyb, int nsub, int nslots) {
    if (pl->d_start && pl->key[0] == yb0 && pl->key[1] == nyb && pl->key[2] == nsub && pl->key[3] == nslots) return BBX_OK;
    int per = nslots / nsub; if (per < 1) per = 1;
    int* len = (int*)malloc((size_t)(nyb + 1) * sizeof(int));
    if (!len) return BBX_ERR_NOMEM;
    int nch = 0, rem = nyb;
    while (rem > 0) {
        int sz = (2 * rem) / (3 * per); if (sz < 2) sz = 2;
        for (int i = 0; i < per && rem > 0; i++) { const int l = sz < rem ? sz : rem; len[nch++] = l; rem -= l; }
    }
    int* start = (int*)malloc((size_t)(nch + 1) * sizeof(int));
    int2* tasks = (int2*)malloc((size_t)nch * nsub * sizeof(int2));
    if (!start || !tasks) { free(len); free(start); free(tasks); return BBX_ERR_NOMEM; }
    start[0] = yb0;
    for (int c = 0; c < nch; c++) start[c + 1] = start[c] + len[c];
    int nt = 0;
    for (int c = 0; c < nch; c++)                                   // len[] is non-increasing: chunk-major = longest first
        for (int sub = 0; sub < nsub; sub++) tasks[nt++] = make_int2(sub, c);
    if (pl->d_start) { (void)hipDeviceSynchronize(); (void)hipFree(pl->d_start); (void)hipFree(pl->d_tasks); pl->d_start = nullptr; pl->d_tasks = nullptr; }
    hipError_t e = hipMalloc((void**)&pl->d_start, (size_t)(nch + 1) * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&pl->d_tasks, (size_t)nt * sizeof(int2));
    if (e == hipSuccess) e = hipMemcpy(pl->d_start, start, (size_t)(nch + 1) * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(pl->d_tasks, tasks, (size_t)nt * sizeof(int2), hipMemcpyHostToDevice);
    free(len); free(start); free(tasks);
    if (e != hipSuccess) return bbx_hip_fail(ctx, e, "chunk plan", __LINE__);
    pl->key[0] = yb0; pl->key[1] = nyb; pl->key[2] = nsub; pl->key[3] = nslots; pl->nch = nch; pl->ntasks = nt;
    return BBX_OK;
}

// The frame call's work arrays in the WS_CAND slot, every region named once, in this order (a unit: nsub P::UNIT entries):
//   T[0..3]     row-transformed N, R, Vn, Vr           U[0..3]    k_img_cols' and k_var_cols' results for k_final_rows
//   cP          the PSF spectra (Pn^, Pr^) as float4: two units; prepared reference PSF: Pn^ alone as float2, one unit
//   K2n, K2r    row-transformed (kn^2)^, (kr^2)^       HSn, HSr   halo rows of the chunks: [nsub][nch][HP]
//   Qdft        row DFTs of the stamps (prepared reference PSF: of the new frame's only)
//   d_sc, (16-byte round-up,) fs_partial, sub_sc, kchk (small grid: [nsub][2][2] energies of the window check)
// The small grid's arrays Ksm, Us lie in U[1], U[2], free until k_img_cols writes them; where k_img_cols itself emits the
// samples (fuse), both in the one unit of cP, which then holds nothing else.
template <class P> struct frame_ws {
    float2 *T[4], *U[4]; float4* cP; float2 *K2n, *K2r, *HSn, *HSr, *Qdft; zscal* d_sc; double* fs_partial; sub_scal* sub_sc; float* kchk;
    float2 *Ksm, *Us;
    size_t bytes;                                           // of the slot, 4096 spare bytes included (the round-up comes out of them)
    template <class X> static void take(uintptr_t& p, X*& m, size_t nbytes) { m = (X*)p; p += nbytes; }
    frame_ws() = default;
    frame_ws(void* base, int nsub, int nch, int S, bool ref_psf, bool fuse) {       // base: the slot, or nullptr to ask for [bytes] alone
        const size_t unit = (size_t)nsub * P::UNIT * sizeof(float2), hunit = (size_t)nsub * nch * P::HP * sizeof(float2);
        uintptr_t p = (uintptr_t)base;
        for (float2*& t : T) take(p, t, unit);
        for (float2*& u : U) take(p, u, unit);
        take(p, cP, (ref_psf ? 1 : 2) * unit);
        take(p, K2n, unit); take(p, K2r, unit);
        take(p, HSn, hunit); take(p, HSr, hunit);
        take(p, Qdft, (ref_psf ? 1 : 2) * (size_t)nsub * S * P::HP * sizeof(float2));
        take(p, d_sc, (size_t)nsub * sizeof(zscal));
        const size_t pad = (0 - p) & 15; p += pad;
        take(p, fs_partial, 5 * (size_t)nsub * P::G * sizeof(double));
        take(p, sub_sc, (size_t)nsub * sizeof(sub_scal));
        take(p, kchk, 4 * (size_t)nsub * sizeof(float));
        bytes = p - (uintptr_t)base - pad + 4096;
        Ksm = U[1]; Us = U[2];
        if constexpr (small_of<P>::ok) {
            typedef typename small_of<P>::type PK;
            constexpr size_t M = PK::L, HM = PK::H, HMP = (HM + 7) / 8 * 8;
            static_assert(2 * HM * M + 2 * M * HMP <= P::UNIT && P::L % PK::L == 0 && M % P::NL == 0, "small-grid arrays fit a unit, both together");
            if (fuse) { Ksm = (float2*)cP; Us = (float2*)((uintptr_t)Ksm + (size_t)nsub * 2 * HM * M * sizeof(float2)); }
        }
    }
    // the once-per-run fills of the prepared reference work at the head of the slot, before the frames lay it out in full: the
    // reference's row pass in T[1], T[3] (the T arrays lead the layout), the row DFTs of its stamps in a Qdft that is all there is
    static frame_ws ref_rows(void* base, int nsub) { frame_ws w(base, nsub, 0, 0, false, false); w.bytes = (uintptr_t)w.U[0] - (uintptr_t)base; return w; }
    static frame_ws ref_psf(void* base, int nsub, int S) { frame_ws w{}; w.Qdft = (float2*)base; w.bytes = (size_t)nsub * S * P::HP * sizeof(float2); return w; }
};

#ifndef Z3_LDS_PAD
#define Z3_LDS_PAD 0           // experiments: extra dynamic LDS per workgroup (forces one workgroup per CU)
#endif
template <class P> constexpr size_t lds_bytes() { return (size_t)P::NL * P::LS * sizeof(float2) + aux_bytes<P>() + Z3_LDS_PAD; }
template <class P, class PK> constexpr size_t lds_ks_rows_bytes() { return lds_bytes<P>() + (size_t)P::NL * PK::LS * sizeof(float2) + ks_tab_bytes<PK>(); }
template <class P> constexpr size_t lds_fin_bytes() { return (size_t)(P::NL + 1) * P::LS * sizeof(float2) + aux_bytes<P>() + Z3_LDS_PAD; }
// dynamic-LDS attribute of the kernels, once per context (= per device and issuing thread) and sub-image side: every kernel
// launched with dynamic LDS is named here, in the group of its byte count
template <class... K> static hipError_t lds_optin(size_t bytes, K... kern) {
    hipError_t e = hipSuccess;
    ((e = e != hipSuccess ? e : hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes)), ...);
    return e;
}
template <class P> static int lds_attrs(bbx_ctx* ctx) {
    if (ctx->zogy3_attr_L == P::L) return BBX_OK;
    BBX_HIP(lds_optin(lds_bytes<P>(), k_psf_cols<P, false>, k_psf_cols<P, false, true>, k_refpsf_cols<P>, k_psf_rows<P>, k_cols_fwd<P>, k_img_rows<P>,
                      k_img_rows_one<P, false>, k_img_rows_one<P, true>, k_img_cols<P, false>, k_img_cols<P, true>, k_img_cols<P, true, 1>,
                      k_var_cols<P, false>, k_var_cols<P, true>));
    BBX_HIP(lds_optin(lds_fin_bytes<P>(), k_final_rows<P>));
    if constexpr (small_of<P>::ok) {
        typedef typename small_of<P>::type PK;
        BBX_HIP(lds_optin(lds_bytes<P>(), k_psf_cols<P, true>, k_img_cols<P, true, 2>));
        BBX_HIP(lds_optin(lds_ks_rows_bytes<P, PK>(), k_ks_rows<P, PK>));
    }
    ctx->zogy3_attr_L = P::L;
    return BBX_OK;
}
// frames whose groups of four pixels are aligned and never straddle a sub-image edge: the 16-byte paths of the row kernels
template <class P> static bool rows_vec4(int nx, int size, int border, const void* a, const void* b, const void* c, const void* d) {
    return size % 4 == 0 && border % 4 == 0 && nx % 4 == 0 && P::L % 4 == 0 && ((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) % 16 == 0;
}
// can a mini sigma image be read in aligned groups of four pixels inside one patch, at most one interval step inside a group
// (boxes wider than 3 pixels)?
static inline bool spl_vec4(const bbx_spl& sp) { return sp.pw % 4 == 0 && 3 * sp.nx1 < sp.dx; }
// cut + row pass of one frame and its variance image -> (Ta, Tva); sigma: a frame (d_sig) or a mini image (sp: its cubic
// table is made first, in [tab])
template <class P>
static void rows_one(bbx_ctx* ctx, const float2* tw, int ny, int nx, int size, int border, const float* d_img, const float* d_sig, const bbx_spl* sp, float4* tab,
                     float2* Ta, float2* Tva, hipStream_t s) {
    const int nsx = nx / size, nsub = (ny / size) * nsx;
    frame1_args fa; fa.a = d_img; fa.sa = d_sig; fa.ny = ny; fa.nx = nx; fa.size = size; fa.border = border; fa.nsx = nsx;
    const dim3 grow = grid8(P::LB, nsub);
    if (sp) {
        bbx_spl t = *sp;
        t.poly = tab;
        hipLaunchKernelGGL(k_spl_polytable, dim3((t.cnx + 255) / 256, ny), dim3(256), 0, s, t, ny, tab);
        BBX_LAUNCH_TIMED(ctx, BBX_PROF_Z_IMG_ROWS, (k_img_rows_one<P, true>), grow, dim3(P::LIGHT_THREADS), lds_bytes<P>(), s, fa, tw, Ta, Tva, nsub, t);
    } else
        BBX_LAUNCH_TIMED(ctx, BBX_PROF_Z_IMG_ROWS, (k_img_rows_one<P, false>), grow, dim3(P::LIGHT_THREADS), lds_bytes<P>(), s, fa, tw, Ta, Tva, nsub, bbx_spl{});
}
static inline size_t spl_table_bytes(const bbx_spl& sp, int ny) { return ((size_t)ny * sp.cnx * sizeof(float4) + 255) & ~(size_t)255; }
// the reference's spectra into a caller's buffer [2][nsub][UNIT] (R^, then Vr^; C layout, a unit holds G NL L <= UNIT entries):
// the row pass into the T[1] / T[3] work arrays, then the column pass of each (bbx_zogy_refrows_fill).  The two column
// launches are not timed: the profile slots count the launches of a frame.
template <class P>
static int fill_ref_rows(bbx_ctx* ctx, const float2* d_tw, int ny, int nx, int size, int border, const float* d_ref, const float* d_sig_ref, const bbx_spl* spr,
                         float2* rows, hipStream_t s) {
    if (!rows_vec4<P>(nx, size, border, d_ref, d_sig_ref, rows, nullptr) || (spr && !spl_vec4(*spr))) return BBX_ERR_ARG;
    int rc = lds_attrs<P>(ctx); if (rc) return rc;
    float4* tab = nullptr;
    if (spr) { tab = (float4*)bbx_ws(ctx, WS_ZSPL, spl_table_bytes(*spr, ny), &rc); if (rc) return rc; }
    const int nsub = (ny / size) * (nx / size);
    const auto w = frame_ws<P>::ref_rows(bbx_ws(ctx, WS_CAND, frame_ws<P>::ref_rows(nullptr, nsub).bytes, &rc), nsub); if (rc) return rc;
    rows_one<P>(ctx, d_tw, ny, nx, size, border, d_ref, d_sig_ref, spr, tab, w.T[1], w.T[3], s);
    hipLaunchKernelGGL(k_cols_fwd<P>, grid8(P::G, nsub), dim3(P::THREADS), lds_bytes<P>(), s, w.T[1], d_tw, rows, nsub);
    hipLaunchKernelGGL(k_cols_fwd<P>, grid8(P::G, nsub), dim3(P::THREADS), lds_bytes<P>(), s, w.T[3], d_tw, rows + (size_t)nsub * P::UNIT, nsub);
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}
// the reference PSF's spectra Pr^ into a caller's buffer [nsub][G][NL L] (C layout; bbx_zogy_refpsf_fill): the row DFTs of the
// reference's stamps into the context's work array, then pass 1 of k_psf_cols on them.  Not timed, as fill_ref_rows.
template <class P>
static int fill_ref_psf(bbx_ctx* ctx, const float2* d_tw, int nsub, const float* d_psf_r, int S, float2* out, hipStream_t s) {
    int rc = lds_attrs<P>(ctx); if (rc) return rc;
    const auto w = frame_ws<P>::ref_psf(bbx_ws(ctx, WS_CAND, frame_ws<P>::ref_psf(nullptr, nsub, S).bytes, &rc), nsub, S); if (rc) return rc;
    hipLaunchKernelGGL(k_psf_rowdft<P>, dim3((P::H + 255) / 256, (S + ZQ_J - 1) / ZQ_J, nsub), dim3(256), 0, s, d_psf_r, d_psf_r, S, d_tw, w.Qdft, nsub);
    hipLaunchKernelGGL(k_refpsf_cols<P>, grid8(P::G, nsub), dim3(P::THREADS), lds_bytes<P>(), s, w.Qdft, S, d_tw, out, nsub);
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}

// Which kernels a frame call runs: decided once at the top of run() from its arguments and the context, before anything is queued.
struct frame_path {
    bool vec4, spl, two;    // row pass: its 16-byte paths (rows_vec4); sigma maps read off their mini images; the two-image kernel k_img_rows
    bool rows, psf;         // prepared reference rows; prepared reference PSF spectra (only with rows: zogy_frame_entry)
    bool win; int wh, wb, nyb_psf;  // row window of k_n, k_r: half-height in rows (no window: L) and row blocks; row blocks of k_psf_rows / k_ks_rows
    bool ks, fuse;          // k_n, k_r on the small grid; k_img_cols forms Pn^ and the grid's samples itself, no k_psf_cols at all (ks && psf)
};
// cut + row pass of the frames -> T[0..3] (prepared reference rows: of the new frame alone -> T[0], T[2])
template <class P>
static int launch_rows(bbx_ctx* ctx, const frame_path& pa, const frame_ws<P>& w, const float2* tw, int ny, int nx, int size, int border, const float* d_new,
                       const float* d_ref, const float* d_sig_new, const float* d_sig_ref, const bbx_spl* spn, const bbx_spl* spr, hipStream_t s) {
    if (pa.two) {
        const int nsx = nx / size, nsub = (ny / size) * nsx;
        const dim3 grow = grid8(P::LB, nsub);
        frame_args fa; fa.a = d_new; fa.b = d_ref; fa.sa = nullptr; fa.sb = nullptr; fa.ny = ny; fa.nx = nx; fa.size = size; fa.border = border; fa.nsx = nsx;
        fa.vec4 = pa.vec4 ? 1 : 0;
        BBX_LAUNCH_TIMED(ctx, BBX_PROF_Z_IMG_ROWS, k_img_rows<P>, grow, dim3(P::LIGHT_THREADS), lds_bytes<P>(), s, fa, tw, w.T[0], w.T[1], nsub);
        fa.sa = d_sig_new; fa.sb = d_sig_ref;
        BBX_LAUNCH_TIMED(ctx, BBX_PROF_Z_IMG_ROWS, k_img_rows<P>, grow, dim3(P::LIGHT_THREADS), lds_bytes<P>(), s, fa, tw, w.T[2], w.T[3], nsub);
        return BBX_OK;
    }
    char* tab = nullptr; size_t nbn = 0;                     // mini images: their cubic tables, the new frame's first
    if (pa.spl) {
        int rc;
        nbn = spl_table_bytes(*spn, ny);
        tab = (char*)bbx_ws(ctx, WS_ZSPL, nbn + (pa.rows ? 0 : spl_table_bytes(*spr, ny)), &rc); if (rc) return rc;
    }
    rows_one<P>(ctx, tw, ny, nx, size, border, d_new, d_sig_new, spn, (float4*)tab, w.T[0], w.T[2], s);
    if (!pa.rows) rows_one<P>(ctx, tw, ny, nx, size, border, d_ref, d_sig_ref, spr, (float4*)(tab + nbn), w.T[1], w.T[3], s);
    return BBX_OK;
}

// small grid: column pass and row pass of k_n, k_r on the samples in Ksm -> K2r, K2n.  The profile slots count the launches of a
// frame: after k_psf_cols (its COLS slot) the two are one BBX_PROF_Z_PSF_ROWS entry, after k_img_cols (fuse) COLS and ROWS.
template <class P>
static void launch_ks(bbx_ctx* ctx, const frame_path& pa, const frame_ws<P>& w, const float2* tw, int nsub, hipStream_t s) {
    if constexpr (small_of<P>::ok) {
        typedef typename small_of<P>::type PK;
        constexpr int M = PK::L, NG = (PK::H + PK::NL - 1) / PK::NL;
        hipEvent_t c0 = nullptr, c1 = nullptr, r0 = nullptr, r1 = nullptr;
        if (pa.fuse) bbx_prof_events(ctx, BBX_PROF_Z_PSF_COLS, &c0, &c1);
        else bbx_prof_start(ctx, BBX_PROF_Z_PSF_ROWS, s);
        hipExtLaunchKernelGGL((k_ks_cols<P, PK>), dim3((unsigned)(NG * 2 * nsub)), dim3(Z3_KS_THREADS), lds_ks_cols_bytes<PK>(), s, c0, c1, 0, w.Ksm, tw, w.Us,
                              w.kchk, nsub, pa.wh);
        if (pa.fuse) bbx_prof_events(ctx, BBX_PROF_Z_PSF_ROWS, &r0, &r1);
        hipExtLaunchKernelGGL((k_ks_rows<P, PK>), grid8(pa.nyb_psf, nsub), dim3(P::LIGHT_THREADS), (lds_ks_rows_bytes<P, PK>()), s, r0, r1, 0, w.Us,
                              1.0f / ((float)M * (float)M), tw, w.K2r, w.K2n, nsub, pa.nyb_psf, pa.wb, w.d_sc, w.fs_partial, w.sub_sc, ctx->d_err, w.kchk);
        if (!pa.fuse) bbx_prof_stop(ctx, s);
    }
}

template <class P>
static int run(bbx_ctx* ctx, const float2* tw, zogy_chunk_plan* plan, int ny, int nx, int size, int border, const float* d_new, const float* d_ref,
               const float* d_sig_new, const float* d_sig_ref, const bbx_spl* spn, const bbx_spl* spr, const float* d_psf_n, const float* d_psf_r, int S, const float* h_scal,
               float* d_D, float* d_S, float* d_Scorr, float* d_Fpsf, float* d_Fpsferr, hipStream_t s) {
    const int nsy = ny / size, nsx = nx / size, nsub = nsy * nsx;
    frame_path pa;
    pa.vec4 = rows_vec4<P>(nx, size, border, d_new, d_ref, d_sig_new, d_sig_ref);
    pa.spl = spn != nullptr;
    pa.two = !pa.spl && !pa.vec4;
#ifdef Z3_ROWS_SPLIT
    pa.two = !pa.spl;
#endif
    const float2 *ref_rows = ctx->zrows.buf, *ref_psf = ctx->zpsf.buf;      // prepared reference (checked by zogy_frame_entry)
    pa.rows = ref_rows != nullptr; pa.psf = ref_psf != nullptr;
    // prepared rows come in the layout of the one-image row kernel; mini images are read in aligned groups of four pixels
    if (pa.rows && (!pa.vec4 || pa.two)) return BBX_ERR_ARG;
    if (pa.spl && (!pa.vec4 || !spl_vec4(*spn) || (!pa.rows && !spl_vec4(*spr)))) return BBX_ERR_ARG;
    // Row window of the matched-filter kernels k_n, k_r (real space): they are as compact as the PSFs they are made
    // of, so only 2 wh of their L rows go through the inverse row pass, the squares and the forward row pass; the rest
    // is below float32 rounding (checked on the device, Z3_KWIN_TOL).  wh: a multiple of NL; W = 2 wh >= 4 S + 32.
    pa.wh = P::L;                                           // 2 wh >= L: no window
    if (!ctx->zogy_kwin_off && P::L % P::NL == 0) {
        int w = ((4 * S + 32) / 2 + P::NL - 1) / P::NL * P::NL;
        if (w < 32) w = (32 + P::NL - 1) / P::NL * P::NL;
        if (2 * w < P::L) pa.wh = w;
    }
    pa.win = 2 * pa.wh < P::L;
    pa.wb = pa.win ? pa.wh / P::NL : 0; pa.nyb_psf = pa.win ? 2 * pa.wb : P::LB;
    // Small grid: inside the window k_n, k_r are given by every F-th frequency of their spectra, so their way back to real
    // space runs at side M = L / F (1 / F^2 of the work); taken where the side has a plan and the window leaves a guard band
    // of a row block or more below M / 2 (L = 1400: F = 5, M = 280).  BBX_OPT_ZOGY_KSMALL_OFF: the full grid, as the sides without.
    pa.ks = false;
    if constexpr (small_of<P>::ok) pa.ks = pa.win && !ctx->zogy_ksmall_off && small_of<P>::type::L / 2 - pa.wh >= P::NL;
    pa.fuse = pa.ks && pa.psf;
    // chunks of the final kernel (chunk_plan; cached with the twiddle table)
    const int yb0 = border / P::NL, yb1 = (border + size - 1) / P::NL, nyb = yb1 - yb0 + 1;
    const int nslots = 2 * (ctx->num_cus > 0 ? ctx->num_cus : 256);
    int rc = chunk_plan(ctx, plan, yb0, nyb, nsub, nslots); if (rc) return rc;
    const int nch = plan->nch;
    const chunk_args ch{plan->d_start, nch};
    const size_t bytes = frame_ws<P>(nullptr, nsub, nch, S, pa.psf, pa.fuse).bytes;
    const frame_ws<P> w(bbx_ws(ctx, WS_CAND, bytes, &rc), nsub, nch, S, pa.psf, pa.fuse); if (rc) return rc;
    BBX_HIP(hipMemcpyAsync(w.d_sc, h_scal, (size_t)nsub * sizeof(zscal), hipMemcpyHostToDevice, s));      // pageable source: staged before the call returns
    const size_t lds = lds_bytes<P>(), lds_fin = lds_fin_bytes<P>();
    rc = lds_attrs<P>(ctx); if (rc) return rc;
    const float inv_n2 = 1.0f / ((float)P::L * (float)P::L);
    const dim3 gcol = grid8(P::G, nsub), blk(P::THREADS);
    // the PSFs: row DFTs of the stamps; then Pn^, Pr^ -> cP and (kn^2)^, (kr^2)^ row-transformed -> K2n, K2r (T layout: their
    // column pass is inside k_var_cols), on the full grid or the small one -- or nothing more here (fuse)
    BBX_LAUNCH_TIMED(ctx, BBX_PROF_Z_PSF_DFT, k_psf_rowdft<P>, dim3((P::H + 255) / 256, (S + ZQ_J - 1) / ZQ_J, (pa.psf ? 1 : 2) * nsub), dim3(256), 0, s, d_psf_n, d_psf_r, S, tw, w.Qdft, nsub);
    auto psf_cols = [&](auto kern, float2* a, float2* b) {
        BBX_LAUNCH_TIMED(ctx, BBX_PROF_Z_PSF_COLS, kern, gcol, blk, lds, s, w.Qdft, S, w.d_sc, tw, w.cP, ref_psf, a, b, w.fs_partial, nsub, pa.wh);
    };
    if (!pa.ks) {
        if (pa.psf) psf_cols(k_psf_cols<P, false, true>, w.U[0], w.U[1]);
        else psf_cols(k_psf_cols<P, false>, w.U[0], w.U[1]);
        BBX_LAUNCH_TIMED(ctx, BBX_PROF_Z_PSF_ROWS, k_psf_rows<P>, grid8(pa.nyb_psf, nsub), dim3(P::LIGHT_THREADS), lds, s, w.U[1], w.U[0], inv_n2, tw, w.K2r, w.K2n, nsub,
                         pa.nyb_psf, pa.wb, w.d_sc, w.fs_partial, w.sub_sc, ctx->d_err);
    } else if (!pa.fuse) {
        if constexpr (small_of<P>::ok) psf_cols(k_psf_cols<P, true>, (float2*)w.kchk, w.Ksm);
        launch_ks<P>(ctx, pa, w, tw, nsub, s);
    }
    rc = launch_rows<P>(ctx, pa, w, tw, ny, nx, size, border, d_new, d_ref, d_sig_new, d_sig_ref, spn, spr, s); if (rc) return rc;
    // D, Sn, Sr; V_S.  Prepared reference: R^, Vr^ come column-transformed (C layout).  k_img_cols<P, PREP, PPSF>: PPSF = 1
    // reads the prepared Pr^, 2 forms Pn^ as well and feeds the small grid (fuse)
    const float2 *TR = pa.rows ? ref_rows : w.T[1], *TVr = pa.rows ? ref_rows + (size_t)nsub * P::UNIT : w.T[3];
    const psf_fuse_args pf = pa.fuse ? psf_fuse_args{w.Qdft, S, w.kchk, w.Ksm, w.fs_partial} : psf_fuse_args{nullptr, 0, nullptr, nullptr, nullptr};
    auto img_cols = [&](auto kern) {
        BBX_LAUNCH_TIMED(ctx, BBX_PROF_Z_IMG_COLS, kern, gcol, blk, lds, s, w.T[0], TR, pa.fuse ? nullptr : w.cP, ref_psf, w.d_sc, tw, w.U[0], w.U[1], w.U[2], w.HSn, w.HSr,
                         nsub, ch, pf);
    };
    if (!pa.rows) img_cols(k_img_cols<P, false>);
    else if (!pa.psf) img_cols(k_img_cols<P, true>);
    else if (!pa.fuse) img_cols(k_img_cols<P, true, 1>);
    else {
        if constexpr (small_of<P>::ok) img_cols(k_img_cols<P, true, 2>);
        launch_ks<P>(ctx, pa, w, tw, nsub, s);
    }
    auto var_cols = [&](auto kern) {
        BBX_LAUNCH_TIMED(ctx, BBX_PROF_Z_VAR_COLS, kern, gcol, dim3(P::VAR_THREADS), lds, s, w.T[2], TVr, w.K2n, w.K2r, tw, w.U[3], w.sub_sc, nsub, pa.wh,
                         &ctx->d_counters[CNT_TICKET], pa.ks ? w.kchk : nullptr, ctx->d_err);
    };
    if (pa.rows) var_cols(k_var_cols<P, true>);
    else var_cols(k_var_cols<P, false>);
    out_args oa; oa.D = d_D; oa.S = d_S; oa.Scorr = d_Scorr; oa.Fpsf = d_Fpsf; oa.Fpsferr = d_Fpsferr;
    oa.ny = ny; oa.nx = nx; oa.size = size; oa.border = border; oa.nsx = nsx; oa.vec4 = 0;
    const dim3 gfin = grid8(plan->ntasks < nslots ? plan->ntasks : nslots, 1);
    // transient candidates on request (bbx_zogy_candidates): listed by the kernel that writes Scorr
    float cand_thr = 0.f; uint32_t* cand_list = nullptr; uint32_t cand_cap = 0;
    int32_t* cand_cnt = &ctx->d_counters[CNT_ZCAND];
    ctx->zcand_img = nullptr;
    if (ctx->zcand_thr > 0.f && (size_t)ny * nx < 0xffffffffull) {
        cand_cap = (uint32_t)bbx_cand_cap((size_t)ny * nx);
        cand_list = (uint32_t*)bbx_ws(ctx, WS_ZCAND, (size_t)cand_cap * sizeof(uint32_t), &rc); if (rc) return rc;
        BBX_HIP(hipMemsetAsync(cand_cnt, 0, sizeof(int32_t), s));
        cand_thr = ctx->zcand_thr;
    }
    BBX_LAUNCH_TIMED(ctx, BBX_PROF_ZOGY_FINAL, k_final_rows<P>, gfin, dim3(P::FIN_THREADS), lds_fin, s, w.U[0], w.U[3], w.U[1], w.U[2], w.HSn, w.HSr, w.d_sc, w.sub_sc,
                     inv_n2, tw, oa, ch, plan->d_tasks, plan->ntasks, &ctx->d_counters[CNT_TICKET], nsub, cand_thr, cand_list, cand_cnt, cand_cap,
                     ctx->d_err);
    if (cand_thr > 0.f) { ctx->zcand_img = d_Scorr; ctx->zcand_thr_used = cand_thr; ctx->zcand_npix = (size_t)ny * nx; }
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}

}  // namespace z3

extern "C" int bbx_zogy_frame_supported(int L) { return z3::with_plan(L, 0, [](auto) { return 1; }); }
// entries of one sub-image's T / U array, and of its spectrum in C layout: G column groups of NL lines of L
static size_t bbx_zogy3_unit(int L) { return z3::with_plan(L, (size_t)0, [](auto p) { return decltype(p)::UNIT; }); }
static size_t bbx_zogy3_cunit(int L) { return z3::with_plan(L, (size_t)0, [](auto p) { return (size_t)decltype(p)::G * decltype(p)::NL * decltype(p)::L; }); }

// ---- entry points (include/bbx.h) ------------------------------------------------------------------------------------
// what the context keeps for bbx_zogy_frame across calls: the twiddle table of the sub-image side, the chunk plan of the geometry
struct zogy_frame_tables { float2* d_tw; int L; z3::zogy_chunk_plan plan; };

void bbx_zogy_frame_release(bbx_ctx* ctx) {          // called by bbx_ctx_destroy
    if (!ctx || !ctx->zogy_frame_state) return;
    zogy_frame_tables* st = (zogy_frame_tables*)ctx->zogy_frame_state;
    if (st->d_tw) (void)hipFree(st->d_tw);
    if (st->plan.d_start) (void)hipFree(st->plan.d_start);
    if (st->plan.d_tasks) (void)hipFree(st->plan.d_tasks);
    free(st);
    ctx->zogy_frame_state = nullptr;
}

#ifdef Z3_STAMPS
// diagnostic builds: buf = device buffer of 6 * Z3_STAMP_WGS * 16 uint64 (or NULL: stamps off)
extern "C" int bbx_z3_stamps(void* buf) {
    unsigned long long* p = (unsigned long long*)buf;
    return hipMemcpyToSymbol(HIP_SYMBOL(z3::g_z3_stamps), &p, sizeof(p)) == hipSuccess ? BBX_OK : BBX_ERR_HIP;
}
#endif

extern "C" int bbx_zogy_candidates(bbx_ctx* ctx, float thr) {
    if (!ctx || !(thr >= 0.f)) return BBX_ERR_ARG;
    ctx->zcand_thr = thr;
    ctx->zcand_img = nullptr;
    return BBX_OK;
}

// the context's tables, with the twiddle table for sub-images of side L
static int zogy_tables(bbx_ctx* ctx, int L, zogy_frame_tables** out) {
    if (!ctx->zogy_frame_state) {
        ctx->zogy_frame_state = calloc(1, sizeof(zogy_frame_tables));
        if (!ctx->zogy_frame_state) return BBX_ERR_NOMEM;
    }
    zogy_frame_tables* st = (zogy_frame_tables*)ctx->zogy_frame_state;
    if (st->L != L) {
        // twiddle table W^m = exp(-2 pi i m / L), float64 on the host, rounded once
        if (st->d_tw) { BBX_HIP(hipDeviceSynchronize()); BBX_HIP(hipFree(st->d_tw)); st->d_tw = nullptr; }
        float2* h = (float2*)malloc((size_t)L * sizeof(float2));
        if (!h) return BBX_ERR_NOMEM;
        for (int m = 0; m < L; m++) {
            const double a = -2.0 * M_PI * (double)m / (double)L;
            h[m] = make_float2((float)cos(a), (float)sin(a));
        }
        hipError_t e = hipMalloc((void**)&st->d_tw, (size_t)L * sizeof(float2));
        if (e == hipSuccess) e = hipMemcpy(st->d_tw, h, (size_t)L * sizeof(float2), hipMemcpyHostToDevice);
        free(h);
        if (e != hipSuccess) return bbx_hip_fail(ctx, e, "twiddle table", __LINE__);
        st->L = L;
    }
    *out = st;
    return BBX_OK;
}

// a frame geometry the frame call takes: whole sub-images of a side with a plan, 4096 at most; aligned: and groups of four
// pixels that never straddle a sub-image edge, as the prepared reference needs them
static bool zgeom_ok(int ny, int nx, int size, int border, bool aligned) {
    if (size < 1 || border < 0 || ny < size || nx < size || ny % size || nx % size) return false;
    const int L = size + 2 * border;
    if (!bbx_zogy_frame_supported(L) || (ny / size) * (nx / size) > 4096) return false;
    return !aligned || (size % 4 == 0 && border % 4 == 0 && nx % 4 == 0 && L % 4 == 0);
}
// prepared reference data (bbx_common.h): made of these very inputs, S and geometry?
static bool zprep_matches(const bbx_zprep& z, const void* id0, const void* id1, int S, int ny, int nx, int size, int border) {
    return z.id[0] == id0 && z.id[1] == id1 && z.S == S && z.geom[0] == ny && z.geom[1] == nx && z.geom[2] == size && z.geom[3] == border;
}
// forget what was prepared; then, with a buffer, remember it and what it was made of (inputs_ok: the caller's own checks of them)
static int zprep_set(bbx_zprep* z, const void* buf, const void* id0, const void* id1, int S, bool inputs_ok, int ny, int nx, int size, int border) {
    *z = bbx_zprep{};
    if (!buf) return BBX_OK;
    if (!inputs_ok || !zgeom_ok(ny, nx, size, border, true) || (uintptr_t)buf % 16) return BBX_ERR_ARG;
    *z = bbx_zprep{(const float2*)buf, {id0, id1}, S, {ny, nx, size, border}};
    return BBX_OK;
}

static int zogy_frame_entry(bbx_ctx* ctx, int ny, int nx, int size, int border, const float* d_new, const float* d_ref,
                            const float* d_sig_new, const float* d_sig_ref, const bbx_spline_image* sig_new, const bbx_spline_image* sig_ref,
                            const float* d_psf_n, const float* d_psf_r, int S,
                            const float* h_scal, float* d_D, float* d_S, float* d_Scorr, float* d_Fpsf, float* d_Fpsferr, void* stream) {
    if (!ctx || !d_new || !d_ref || !d_psf_n || !d_psf_r || !h_scal || !d_D || !d_Scorr || !d_Fpsf || !d_Fpsferr) return BBX_ERR_ARG;
    const int L = size + 2 * border;
    if (!zgeom_ok(ny, nx, size, border, false) || S < 1 || S > L) return BBX_ERR_ARG;
    bbx_spl spn, spr;
    const bool spl = sig_new != nullptr;
    if (spl) {
        int rc = bbx_spl_make(sig_new, ny, nx, &spn); if (rc) return rc;
        rc = bbx_spl_make(sig_ref, ny, nx, &spr); if (rc) return rc;
    }
    // prepared reference rows (bbx_zogy_refrows): only for the very reference, sigma map and geometry they were made of
    if (ctx->zrows.buf && !zprep_matches(ctx->zrows, d_ref, spl ? (const void*)sig_ref->d_coef : (const void*)d_sig_ref, 0, ny, nx, size, border)) return BBX_ERR_ARG;
    // prepared reference PSF spectra (bbx_zogy_refpsf): only with prepared rows, for the very stamps, S and geometry they were made of
    if (ctx->zpsf.buf && (!ctx->zrows.buf || !zprep_matches(ctx->zpsf, d_psf_r, nullptr, S, ny, nx, size, border))) return BBX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    zogy_frame_tables* st;
    int rc = zogy_tables(ctx, L, &st); if (rc) return rc;
    return z3::with_plan(L, BBX_ERR_ARG, [&](auto p) {
        return z3::run<decltype(p)>(ctx, st->d_tw, &st->plan, ny, nx, size, border, d_new, d_ref, d_sig_new, d_sig_ref, spl ? &spn : nullptr, spl ? &spr : nullptr,
                                    d_psf_n, d_psf_r, S, h_scal, d_D, d_S, d_Scorr, d_Fpsf, d_Fpsferr, s);
    });
}

extern "C" int bbx_zogy_frame(bbx_ctx* ctx, int ny, int nx, int size, int border, const float* d_new, const float* d_ref,
                              const float* d_sig_new, const float* d_sig_ref, const float* d_psf_n, const float* d_psf_r, int S,
                              const float* h_scal, float* d_D, float* d_S, float* d_Scorr, float* d_Fpsf, float* d_Fpsferr,
                              void* stream) {
    if (!d_sig_new || !d_sig_ref) return BBX_ERR_ARG;
    return zogy_frame_entry(ctx, ny, nx, size, border, d_new, d_ref, d_sig_new, d_sig_ref, nullptr, nullptr, d_psf_n, d_psf_r, S, h_scal, d_D, d_S, d_Scorr,
                            d_Fpsf, d_Fpsferr, stream);
}

extern "C" int bbx_zogy_frame_mini(bbx_ctx* ctx, int ny, int nx, int size, int border, const float* d_new, const float* d_ref,
                                   const bbx_spline_image* sig_new, const bbx_spline_image* sig_ref, const float* d_psf_n, const float* d_psf_r,
                                   int S, const float* h_scal, float* d_D, float* d_S, float* d_Scorr, float* d_Fpsf, float* d_Fpsferr,
                                   void* stream) {
    if (!sig_new || !sig_ref) return BBX_ERR_ARG;
    return zogy_frame_entry(ctx, ny, nx, size, border, d_new, d_ref, nullptr, nullptr, sig_new, sig_ref, d_psf_n, d_psf_r, S, h_scal, d_D, d_S, d_Scorr,
                            d_Fpsf, d_Fpsferr, stream);
}

// ---- prepared reference rows ---------------------------------------------------------------------------------------
extern "C" size_t bbx_zogy_refrows_bytes(int ny, int nx, int size, int border) {
    if (!zgeom_ok(ny, nx, size, border, true)) return 0;
    return 2 * (size_t)(ny / size) * (nx / size) * bbx_zogy3_unit(size + 2 * border) * sizeof(float2);
}

static int refrows_fill_entry(bbx_ctx* ctx, int ny, int nx, int size, int border, const float* d_ref, const float* d_sig_ref, const bbx_spline_image* sig_ref,
                              void* d_rows, void* stream) {
    if (!ctx || !d_ref || !d_rows || (!d_sig_ref && !sig_ref) || !zgeom_ok(ny, nx, size, border, true)) return BBX_ERR_ARG;
    bbx_spl spr;
    if (sig_ref) { int rc = bbx_spl_make(sig_ref, ny, nx, &spr); if (rc) return rc; }
    const int L = size + 2 * border;
    zogy_frame_tables* st;
    int rc = zogy_tables(ctx, L, &st); if (rc) return rc;
    return z3::with_plan(L, BBX_ERR_ARG, [&](auto p) {
        return z3::fill_ref_rows<decltype(p)>(ctx, st->d_tw, ny, nx, size, border, d_ref, d_sig_ref, sig_ref ? &spr : nullptr, (float2*)d_rows, (hipStream_t)stream);
    });
}

extern "C" int bbx_zogy_refrows_fill(bbx_ctx* ctx, int ny, int nx, int size, int border, const float* d_ref, const float* d_sig_ref, void* d_rows, void* stream) {
    if (!d_sig_ref) return BBX_ERR_ARG;
    return refrows_fill_entry(ctx, ny, nx, size, border, d_ref, d_sig_ref, nullptr, d_rows, stream);
}

extern "C" int bbx_zogy_refrows_fill_mini(bbx_ctx* ctx, int ny, int nx, int size, int border, const float* d_ref, const bbx_spline_image* sig_ref, void* d_rows,
                                          void* stream) {
    if (!sig_ref) return BBX_ERR_ARG;
    return refrows_fill_entry(ctx, ny, nx, size, border, d_ref, nullptr, sig_ref, d_rows, stream);
}

extern "C" int bbx_zogy_refrows(bbx_ctx* ctx, const void* d_rows, int ny, int nx, int size, int border, const float* d_ref, const void* ref_sigma) {
    if (!ctx) return BBX_ERR_ARG;
    return zprep_set(&ctx->zrows, d_rows, d_ref, ref_sigma, 0, d_ref && ref_sigma, ny, nx, size, border);
}

// ---- prepared reference PSF spectra ------------------------------------------------------------------------------
extern "C" size_t bbx_zogy_refpsf_bytes(int ny, int nx, int size, int border) {
    if (!zgeom_ok(ny, nx, size, border, true)) return 0;
    return (size_t)(ny / size) * (nx / size) * bbx_zogy3_cunit(size + 2 * border) * sizeof(float2);
}

extern "C" int bbx_zogy_refpsf_fill(bbx_ctx* ctx, int ny, int nx, int size, int border, const float* d_psf_r, int S, void* d_out, void* stream) {
    if (!ctx || !d_psf_r || !d_out || (uintptr_t)d_out % 16 || !zgeom_ok(ny, nx, size, border, true) || S < 1 || S > size + 2 * border) return BBX_ERR_ARG;
    const int L = size + 2 * border;
    zogy_frame_tables* st;
    int rc = zogy_tables(ctx, L, &st); if (rc) return rc;
    return z3::with_plan(L, BBX_ERR_ARG, [&](auto p) {
        return z3::fill_ref_psf<decltype(p)>(ctx, st->d_tw, (ny / size) * (nx / size), d_psf_r, S, (float2*)d_out, (hipStream_t)stream);
    });
}

extern "C" int bbx_zogy_refpsf(bbx_ctx* ctx, const void* d_spec, int ny, int nx, int size, int border, const float* d_psf_r, int S) {
    if (!ctx) return BBX_ERR_ARG;
    return zprep_set(&ctx->zpsf, d_spec, d_psf_r, nullptr, S, d_psf_r && S >= 1 && (long long)S <= (long long)size + 2LL * border, ny, nx, size, border);
}

// bbx_build_flags (bbx_ctx.hip): any timing / diagnostic switch of this file compiled in?
int bbx_build_flags_zogy(void) {
#if defined(Z3_SKIP_FFT) || defined(Z3_STAMPS) || defined(Z3_FFT2X) || defined(Z3_NO_PREFETCH) || defined(Z3_NO_XCD) || defined(Z3_NO_CONTRACT) || defined(Z3_NO_ZSKIP) || \
    defined(Z3_TWPOW) || defined(Z3_ROWS_SPLIT) || defined(Z3_ROWS_XCD) || defined(Z3_EXACT_SQRT)
    return 2;
#else
    return 0;
#endif
}
