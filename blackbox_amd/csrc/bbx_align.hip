// bbx_align.hip -- registration of the reference on the new frame from the two star lists (the rules are THIS
// PROJECT'S OWN, stated in float64 numpy by tests/test_align_host.py: vote_ref, fit_ref, apply_ref, grid_of, remap_mask_ref).
//
//   bbx_align_vote  : k_vote_select (one workgroup per list: radix selection of the nbright-th key, LDS sort of the selected),
//                     k_vote_hist (one thread per pair, integer atomics on the histogram in global memory: 129 x 129 int32 =
//                     66.6 KB is more than the 64 KB a workgroup may declare statically), k_vote_pick (one workgroup: 3 x 3
//                     block sums, winner, runner-up, far block), k_vote_rows twice (one wave per source of A: count of its
//                     pairs in the winning block, then their emission at the prefix count: row-major order of (rank in A,
//                     rank in B) whatever the order of arrival), k_vote_final (one workgroup: the two medians by an LDS sort)
//   bbx_align_fit   : one workgroup; normal equations in float64 (per-thread partial sums in index order, wave sums by DPP,
//                     wave totals in wave order), Cholesky with the 1e-12 pivot rule by every thread alike, four passes
//   bbx_align_apply : one thread per source, the float64 operations of apply_ref one by one
//   bbx_align_grid  : one thread per lattice node
//   bbx_remap_mask  : four output pixels per thread, one 32-bit store; the edge pixels counted per wave, one integer add each
//
// No float atomics anywhere: same input, same bits.  Every index a kernel reads with is checked against the extent the entry
// was given for that array.
#include "bbx_common.h"

#define AL_BLOCK    1024
#define AL_WAVES    (AL_BLOCK / 64)
#define FIT_BLOCK   512                      // bbx_align_fit: 256 registers per thread hold the 6 x 6 system without spills
#define FIT_WAVES   (FIT_BLOCK / 64)
#define AL_NBRIGHT  BBX_ALIGN_NBRIGHT_MAX
#define AL_CAP      BBX_ALIGN_CAP_MAX

struct al_list { const int32_t* ys; const int32_t* xs; const float* off; const float* flux; const float* err; int n; };
// the selected sources of one list, in rank order: index into the list, integer peak, offset
struct al_sel { int32_t* idx; int32_t* y; int32_t* x; float* oy; float* ox; };
struct al_ws {
    int32_t* hist;                   // [nb * nb]
    int32_t* cnt;                    // [8]: 0, 1 = selected of A, B; 2 .. 6 = wsum, rsum, wy, wx, far sum
    al_sel a, b;                     // [AL_NBRIGHT] each
    int32_t* rowcnt;                 // [AL_NBRIGHT]
    float* pdy; float* pdx;          // [cap]: dy, dx of the pairs written
};

static inline size_t al_up(size_t b) { return (b + 255) / 256 * 256; }
static size_t al_ws_layout(int nb, int cap, char* base, al_ws* w) {
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += al_up(bytes); return p; };
    al_ws t;
    t.hist = (int32_t*)take((size_t)nb * nb * 4);
    t.cnt = (int32_t*)take(8 * 4);
    for (al_sel* s : {&t.a, &t.b}) {
        s->idx = (int32_t*)take(AL_NBRIGHT * 4); s->y = (int32_t*)take(AL_NBRIGHT * 4); s->x = (int32_t*)take(AL_NBRIGHT * 4);
        s->oy = (float*)take(AL_NBRIGHT * 4); s->ox = (float*)take(AL_NBRIGHT * 4);
    }
    t.rowcnt = (int32_t*)take(AL_NBRIGHT * 4);
    t.pdy = (float*)take((size_t)cap * 4); t.pdx = (float*)take((size_t)cap * 4);
    if (w) *w = t;
    return o;
}
static inline bool al_bins(double max_shift, double bin, int* nb) {
    if (!(max_shift > 0.0) || !(bin > 0.0) || !(2.0 * max_shift / bin < 1023.0)) return false;
    *nb = (int)floor(2.0 * max_shift / bin) + 1;
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------
// vote
// ---------------------------------------------------------------------------------------------------------------------
// eligible: flux > 0 and finite, both offsets finite.  key: brighter first, ties to the lower index; unique per source
__device__ __forceinline__ bool vote_key(const al_list& L, int i, unsigned long long* key) {
    const float f = L.flux[i], oy = L.off[2 * (size_t)i], ox = L.off[2 * (size_t)i + 1];
    *key = ((unsigned long long)(~f2key(f)) << 32) | (unsigned)i;
    return f > 0.f && finite_f32(f) && finite_f32(oy) && finite_f32(ox);
}

__global__ __launch_bounds__(AL_BLOCK) void k_vote_select(al_list A, al_list B, int nbright, al_ws w) {
    __shared__ unsigned long long s_key[AL_NBRIGHT];
    __shared__ int s_hist[256];
    __shared__ unsigned long long s_prefix;
    __shared__ int s_k, s_n;
    const al_list L = blockIdx.x ? B : A;
    const al_sel S = blockIdx.x ? w.b : w.a;
    const int tid = threadIdx.x;
    if (tid == 0) s_n = 0;
    __syncthreads();
    int c = 0;
    unsigned long long key;
    for (int i = tid; i < L.n; i += AL_BLOCK) c += vote_key(L, i, &key) ? 1 : 0;
    c = wave_sum_i32(c);
    if ((tid & 63) == 0 && c) atomicAdd(&s_n, c);
    __syncthreads();
    const int m = s_n;
    const int k = min(nbright, m);                                   // (uniform)
    if (tid == 0) w.cnt[blockIdx.x] = k;
    if (k == 0) return;
    unsigned long long thr = ~0ull;
    if (m > nbright) {
        // the k-th smallest key, eight bits at a time from the top
        if (tid == 0) { s_prefix = 0; s_k = k; }
        for (int pass = 0; pass < 8; pass++) {
            const int shift = 56 - 8 * pass;
            if (tid < 256) s_hist[tid] = 0;
            __syncthreads();
            const unsigned long long pre = s_prefix;
            for (int i = tid; i < L.n; i += AL_BLOCK)
                if (vote_key(L, i, &key) && (pass == 0 || (key >> (shift + 8)) == (pre >> (shift + 8))))
                    atomicAdd(&s_hist[(int)((key >> shift) & 255)], 1);
            __syncthreads();
            if (tid == 0) {
                int left = s_k, d = 0;
                while (d < 255 && s_hist[d] < left) { left -= s_hist[d]; d++; }
                s_k = left; s_prefix = pre | ((unsigned long long)d << shift);
            }
            __syncthreads();
        }
        thr = s_prefix;
    }
    __syncthreads();
    if (tid == 0) s_n = 0;
    for (int r = tid; r < AL_NBRIGHT; r += AL_BLOCK) s_key[r] = ~0ull;
    __syncthreads();
    for (int i = tid; i < L.n; i += AL_BLOCK)
        if (vote_key(L, i, &key) && key <= thr) {
            const int pos = atomicAdd(&s_n, 1);
            if (pos < AL_NBRIGHT) s_key[pos] = key;                  // (the keys are unique: exactly k of them are <= thr)
        }
    __syncthreads();
    lds_sort<AL_BLOCK>(s_key, AL_NBRIGHT);
    for (int r = tid; r < k; r += AL_BLOCK) {
        const int i = (int)(s_key[r] & 0xffffffffu);
        if (i < L.n) {
            S.idx[r] = i; S.y[r] = L.ys[i]; S.x[r] = L.xs[i];
            S.oy[r] = L.off[2 * (size_t)i]; S.ox[r] = L.off[2 * (size_t)i + 1];
        }
    }
}

// the difference of one pair, float32 as bbx_match_mutual forms it, and its bin
struct vote_pair { float dy, dx; int by, bx; bool ok; };
__device__ __forceinline__ vote_pair vote_form(const al_sel& a, int ra, const al_sel& b, int rb, float ms, float bn, int nb) {
    vote_pair p;
    p.dy = (float)((long long)a.y[ra] - (long long)b.y[rb]) + (a.oy[ra] - b.oy[rb]);
    p.dx = (float)((long long)a.x[ra] - (long long)b.x[rb]) + (a.ox[ra] - b.ox[rb]);
    p.ok = fabsf(p.dy) <= ms && fabsf(p.dx) <= ms;
    p.by = p.bx = 0;
    if (p.ok) {
        p.by = min(max((int)floorf((p.dy + ms) / bn), 0), nb - 1);
        p.bx = min(max((int)floorf((p.dx + ms) / bn), 0), nb - 1);
    }
    return p;
}

__global__ __launch_bounds__(256) void k_vote_hist(al_ws w, float ms, float bn, int nb) {
    const int ra = blockIdx.y, rb = blockIdx.x * 256 + threadIdx.x;
    if (ra >= w.cnt[0] || rb >= w.cnt[1]) return;
    const vote_pair p = vote_form(w.a, ra, w.b, rb, ms, bn, nb);
    if (p.ok) atomicAdd(&w.hist[p.by * nb + p.bx], 1);
}

__device__ __forceinline__ int vote_block_sum(const int32_t* hist, int nb, int j, int i) {
    int s = 0;
    for (int dj = -1; dj <= 1; dj++)
        for (int di = -1; di <= 1; di++) {
            const int jj = j + dj, ii = i + di;
            if (jj >= 0 && jj < nb && ii >= 0 && ii < nb) s += hist[jj * nb + ii];
        }
    return s;
}

__global__ __launch_bounds__(AL_BLOCK) void k_vote_pick(al_ws w, int nb, int far) {
    __shared__ unsigned long long s_best[AL_WAVES];
    __shared__ int s_rs, s_fs;
    const int tid = threadIdx.x;
    if (tid == 0) { s_rs = 0; s_fs = 0; }
    const bool any = w.cnt[0] > 0 && w.cnt[1] > 0;                   // (uniform)
    // largest block sum, the lowest cell index on ties: the key orders by (sum, -index)
    unsigned long long best = 0;
    if (any)
        for (int c = tid; c < nb * nb; c += AL_BLOCK) {
            const unsigned long long key = ((unsigned long long)(unsigned)vote_block_sum(w.hist, nb, c / nb, c % nb) << 32) | (0xffffffffu - (unsigned)c);
            best = key > best ? key : best;
        }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long v = ((unsigned long long)(unsigned)__shfl_xor((int)(best >> 32), o) << 32) | (unsigned)__shfl_xor((int)best, o);
        best = v > best ? v : best;
    }
    if ((tid & 63) == 0) s_best[tid >> 6] = best;
    __syncthreads();
    best = s_best[0];
    for (int k = 1; k < AL_WAVES; k++) best = s_best[k] > best ? s_best[k] : best;
    const int wsum = (int)(best >> 32);
    const int widx = wsum > 0 ? (int)(0xffffffffu - (unsigned)best) : 0;
    const int wy = widx / nb, wx = widx % nb;
    int rs = 0, fs = 0;
    if (any)
        for (int c = tid; c < nb * nb; c += AL_BLOCK) {
            const int j = c / nb, i = c % nb;
            const int ay = abs(j - wy), ax = abs(i - wx);
            if (ay > 2 || ax > 2 || ay > far || ax > far) {
                const int s = vote_block_sum(w.hist, nb, j, i);
                if (ay > 2 || ax > 2) rs = max(rs, s);
                if (ay > far || ax > far) fs = max(fs, s);
            }
        }
    if (rs) atomicMax(&s_rs, rs);
    if (fs) atomicMax(&s_fs, fs);
    __syncthreads();
    if (tid == 0) { w.cnt[2] = wsum; w.cnt[3] = s_rs; w.cnt[4] = wy; w.cnt[5] = wx; w.cnt[6] = s_fs; }
}

// one wave per selected source of A.  phase 0: rowcnt[ra] = its pairs in the winning block.  phase 1: they are written at
// the count of the rows before + their rank in the row, up to cap
__global__ __launch_bounds__(256) void k_vote_rows(al_ws w, float ms, float bn, int nb, int phase, int cap, int32_t* __restrict__ pairs) {
    const int lane = threadIdx.x & 63;
    const int ra = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int na = w.cnt[0], nbs = w.cnt[1];
    if (ra >= na) return;                                            // (uniform per wave)
    const int wsum = w.cnt[2], wy = w.cnt[4], wx = w.cnt[5];
    int base = 0;
    if (phase == 1) {
        for (int r = lane; r < ra; r += 64) base += w.rowcnt[r];
        base = wave_sum_i32(base);
        if (base >= cap) return;
    }
    int count = 0;
    if (wsum > 0)
        for (int r0 = 0; r0 < nbs; r0 += 64) {
            const int rb = r0 + lane;
            bool in = false;
            vote_pair p;
            if (rb < nbs) {
                p = vote_form(w.a, ra, w.b, rb, ms, bn, nb);
                in = p.ok && abs(p.by - wy) <= 1 && abs(p.bx - wx) <= 1;
            }
            const unsigned long long m = __builtin_amdgcn_ballot_w64(in);
            if (phase == 1 && in) {
                const int pos = base + count + __popcll(m & ((1ull << lane) - 1ull));
                if (pos < cap) {
                    pairs[2 * (size_t)pos] = w.a.idx[ra]; pairs[2 * (size_t)pos + 1] = w.b.idx[rb];
                    w.pdy[pos] = p.dy; w.pdx[pos] = p.dx;
                }
            }
            count += __popcll(m);
        }
    if (phase == 0 && lane == 0) w.rowcnt[ra] = count;
}

// median by the project's even-count rule of v[0 .. m) (m <= AL_CAP), NaN for m = 0; s: LDS, AL_CAP keys
__device__ __forceinline__ double vote_median(const float* v, int m, uint32_t* s) {
    int n2 = 2;
    while (n2 < m) n2 <<= 1;
    __syncthreads();
    for (int i = threadIdx.x; i < n2; i += AL_BLOCK) s[i] = i < m ? f2key(v[i]) : 0xffffffffu;
    __syncthreads();
    lds_sort<AL_BLOCK>(s, n2);
    if (m == 0) return __builtin_nan("");
    return 0.5 * ((double)key2f(s[(m - 1) / 2]) + (double)key2f(s[m / 2]));
}

__global__ __launch_bounds__(AL_BLOCK) void k_vote_final(al_ws w, int nmin, int cap, int32_t* __restrict__ info, double* __restrict__ coarse) {
    __shared__ uint32_t s_keys[AL_CAP];
    __shared__ int s_tot;
    const int tid = threadIdx.x;
    if (tid == 0) s_tot = 0;
    __syncthreads();
    const int na = w.cnt[0];
    int c = 0;
    for (int r = tid; r < na; r += AL_BLOCK) c += w.rowcnt[r];
    c = wave_sum_i32(c);
    if ((tid & 63) == 0 && c) atomicAdd(&s_tot, c);
    __syncthreads();
    const int found = s_tot, written = min(found, cap);
    const double my = vote_median(w.pdy, written, s_keys);
    const double mx = vote_median(w.pdx, written, s_keys);
    if (tid == 0) {
        const long long wsum = w.cnt[2], rsum = w.cnt[3], fsum = w.cnt[6];
        const long long gap = wsum - fsum;
        info[0] = (int)wsum; info[1] = (int)rsum; info[2] = w.cnt[4]; info[3] = w.cnt[5]; info[4] = written;
        info[5] = (wsum < nmin || wsum <= rsum || gap <= 0 || gap * gap <= 9 * fsum) ? 1 : 0;
        info[6] = found; info[7] = (int)fsum;
        coarse[0] = my; coarse[1] = mx;
    }
}

extern "C" size_t bbx_align_vote_bytes(int nbright, double max_shift, double bin, int cap) {
    int nb;
    if (nbright < 1 || nbright > AL_NBRIGHT || cap < 1 || cap > AL_CAP || !al_bins(max_shift, bin, &nb)) return 0;
    return al_ws_layout(nb, cap, nullptr, nullptr);
}

extern "C" int bbx_align_vote(bbx_ctx* ctx, int n_a, const int32_t* d_a_ys, const int32_t* d_a_xs, const float* d_a_off, const float* d_a_flux,
                              int n_b, const int32_t* d_b_ys, const int32_t* d_b_xs, const float* d_b_off, const float* d_b_flux, int nbright,
                              double max_shift, double bin, int nmin, int far, int cap, void* d_work, size_t work_bytes, int32_t* d_info,
                              double* d_coarse, int32_t* d_pairs, void* stream) {
    int nb;
    if (!ctx || n_a < 0 || n_b < 0 || nbright < 1 || nbright > AL_NBRIGHT || cap < 1 || cap > AL_CAP || nmin < 0 || far < 0 ||
        !al_bins(max_shift, bin, &nb))
        return BBX_ERR_ARG;
    if (!d_work || !d_info || !d_coarse || !d_pairs) return BBX_ERR_ARG;
    if (n_a > 0 && (!d_a_ys || !d_a_xs || !d_a_off || !d_a_flux)) return BBX_ERR_ARG;
    if (n_b > 0 && (!d_b_ys || !d_b_xs || !d_b_off || !d_b_flux)) return BBX_ERR_ARG;
    al_ws w;
    if (al_ws_layout(nb, cap, (char*)d_work, &w) > work_bytes) return BBX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const al_list A = {d_a_ys, d_a_xs, d_a_off, d_a_flux, nullptr, n_a}, B = {d_b_ys, d_b_xs, d_b_off, d_b_flux, nullptr, n_b};
    const float ms = (float)max_shift, bn = (float)bin;
    BBX_HIP(hipMemsetAsync(w.hist, 0, (size_t)nb * nb * 4, s));
    BBX_HIP(hipMemsetAsync(w.cnt, 0, 8 * 4, s));
    BBX_HIP(hipMemsetAsync(w.rowcnt, 0, AL_NBRIGHT * 4, s));
    BBX_HIP(hipMemsetAsync(d_pairs, 0xff, (size_t)cap * 2 * 4, s));  // (-1, -1) past the pairs written
    hipLaunchKernelGGL(k_vote_select, dim3(2), dim3(AL_BLOCK), 0, s, A, B, nbright, w);
    BBX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_vote_hist, dim3((nbright + 255) / 256, nbright), dim3(256), 0, s, w, ms, bn, nb);
    BBX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_vote_pick, dim3(1), dim3(AL_BLOCK), 0, s, w, nb, far);
    BBX_LAUNCH_CHECK();
    for (int phase = 0; phase < 2; phase++) {
        hipLaunchKernelGGL(k_vote_rows, dim3((nbright + 3) / 4), dim3(256), 0, s, w, ms, bn, nb, phase, cap, d_pairs);
        BBX_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_vote_final, dim3(1), dim3(AL_BLOCK), 0, s, w, nmin, cap, d_info, d_coarse);
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// fit
// ---------------------------------------------------------------------------------------------------------------------
struct fit_args {
    al_list A, B;
    const int32_t* items; int N;
    int ny, nx, nmin;
    float snr_min;
    double clip;
    double* coef; double* stats; uint8_t* kept;
};

// item i: does it qualify, and if so its basis values (1, u, v, u^2, uv, v^2) at the new frame's position and the
// reference's position (X, Y)
__device__ __forceinline__ bool fit_load(const fit_args& a, int i, double* Bv, double* X, double* Y) {
    const int ia = a.items[2 * (size_t)i], ib = a.items[2 * (size_t)i + 1];
    if (ia < 0 || ib < 0 || ia >= a.A.n || ib >= a.B.n) return false;
    const float fa = a.A.flux[ia], ea = a.A.err[ia], fb = a.B.flux[ib], eb = a.B.err[ib];
    const float aoy = a.A.off[2 * (size_t)ia], aox = a.A.off[2 * (size_t)ia + 1];
    const float boy = a.B.off[2 * (size_t)ib], box = a.B.off[2 * (size_t)ib + 1];
    if (!(fa > 0.f && fb > 0.f && fa / ea >= a.snr_min && fb / eb >= a.snr_min && finite_f32(aoy) && finite_f32(aox) && finite_f32(boy) &&
          finite_f32(box)))
        return false;
    const double hy = 0.5 * (double)a.ny, hx = 0.5 * (double)a.nx;
    const double x = (double)a.A.xs[ia] + (double)aox, y = (double)a.A.ys[ia] + (double)aoy;
    const double u = (x - hx) / hx, v = (y - hy) / hy;
    Bv[0] = 1.0; Bv[1] = u; Bv[2] = v; Bv[3] = u * u; Bv[4] = u * v; Bv[5] = v * v;
    *X = (double)a.B.xs[ib] + (double)box; *Y = (double)a.B.ys[ib] + (double)boy;
    return true;
}

template <int NC>
__device__ __forceinline__ void fit_body(const fit_args& a, double* red) {
    const int tid = threadIdx.x;
    const double nan = __builtin_nan("");
    double coef[12];
    for (int k = 0; k < 12; k++) coef[k] = nan;
    double rms_x = nan, rms_y = nan, n_used = 0.0;
    int flags = 0;
    if (a.A.n == 0 || a.B.n == 0) {
        for (int i = tid; i < a.N; i += FIT_BLOCK) a.kept[i] = 0;
        flags = 2;
    } else {
        for (int i = tid; i < a.N; i += FIT_BLOCK) {
            double Bv[6], X, Y;
            a.kept[i] = fit_load(a, i, Bv, &X, &Y) ? 1 : 0;
        }
        for (int pass = 0; pass < 4; pass++) {
            // normal equations over the kept pairs: lower triangle of B^T B, B^T X, B^T Y, the count
            double M[NC * (NC + 1) / 2], bx[NC], by[NC], cnt = 0.0;
            for (int k = 0; k < NC * (NC + 1) / 2; k++) M[k] = 0.0;
            for (int k = 0; k < NC; k++) { bx[k] = 0.0; by[k] = 0.0; }
            for (int i = tid; i < a.N; i += FIT_BLOCK) {              // (a thread only ever touches its own entries of kept)
                double Bv[6], X, Y;
                if (!a.kept[i] || !fit_load(a, i, Bv, &X, &Y)) continue;
                cnt += 1.0;
                int q = 0;
#pragma unroll
                for (int r = 0; r < NC; r++) {
#pragma unroll
                    for (int c = 0; c <= r; c++) M[q++] += Bv[r] * Bv[c];
                    bx[r] += Bv[r] * X; by[r] += Bv[r] * Y;
                }
            }
            cnt = wg_sum_seq<FIT_WAVES>(cnt, red);
#pragma unroll
            for (int k = 0; k < NC * (NC + 1) / 2; k++) M[k] = wg_sum_seq<FIT_WAVES>(M[k], red);
#pragma unroll
            for (int k = 0; k < NC; k++) { bx[k] = wg_sum_seq<FIT_WAVES>(bx[k], red); by[k] = wg_sum_seq<FIT_WAVES>(by[k], red); }
            n_used = cnt;
            if (cnt < (double)max(a.nmin, NC)) { flags |= 2; break; }                  // (every thread holds the same sums)
            // Cholesky, lower factor in place of the triangle; a pivot not above 1e-12 of its diagonal element: not positive definite
            double Lm[NC][NC];
            bool pd = true;
#pragma unroll
            for (int j = 0; j < NC; j++) {
                const double mjj = M[j * (j + 1) / 2 + j];
                double d = mjj;
                for (int k = 0; k < j; k++) d -= Lm[j][k] * Lm[j][k];
                if (!(d > 1e-12 * mjj) || !(fabs(d) < __builtin_huge_val())) { pd = false; break; }
                Lm[j][j] = sqrt(d);
                for (int r = j + 1; r < NC; r++) {
                    double t = M[r * (r + 1) / 2 + j];
                    for (int k = 0; k < j; k++) t -= Lm[r][k] * Lm[j][k];
                    Lm[r][j] = t / Lm[j][j];
                }
            }
            if (!pd) { flags |= 4; break; }
            double c[12];
            for (int k = 0; k < 12; k++) c[k] = 0.0;
#pragma unroll
            for (int side = 0; side < 2; side++) {
                const double* rhs = side ? by : bx;
                double z[NC];
                for (int r = 0; r < NC; r++) {
                    double t = rhs[r];
                    for (int k = 0; k < r; k++) t -= Lm[r][k] * z[k];
                    z[r] = t / Lm[r][r];
                }
                for (int r = NC - 1; r >= 0; r--) {
                    double t = z[r];
                    for (int k = r + 1; k < NC; k++) t -= Lm[k][r] * c[6 * side + k];
                    c[6 * side + r] = t / Lm[r][r];
                }
            }
            // residuals of the kept pairs, their sums of squares, the clip
            double sx = 0.0, sy = 0.0;
            for (int i = tid; i < a.N; i += FIT_BLOCK) {
                double Bv[6], X, Y;
                if (!a.kept[i] || !fit_load(a, i, Bv, &X, &Y)) continue;
                double rx = X, ry = Y;
#pragma unroll
                for (int k = 0; k < NC; k++) { rx = rx - c[k] * Bv[k]; ry = ry - c[6 + k] * Bv[k]; }
                sx += rx * rx; sy += ry * ry;
            }
            sx = wg_sum_seq<FIT_WAVES>(sx, red);
            sy = wg_sum_seq<FIT_WAVES>(sy, red);
            for (int k = 0; k < 12; k++) coef[k] = c[k];
            rms_x = sqrt(sx / cnt); rms_y = sqrt(sy / cnt);
            if (pass == 3) break;                                    // (the set the last solve used is the one reported)
            const double lim = a.clip * a.clip * ((sx + sy) / cnt);
            for (int i = tid; i < a.N; i += FIT_BLOCK) {
                double Bv[6], X, Y;
                if (!a.kept[i] || !fit_load(a, i, Bv, &X, &Y)) continue;
                double rx = X, ry = Y;
#pragma unroll
                for (int k = 0; k < NC; k++) { rx = rx - c[k] * Bv[k]; ry = ry - c[6 + k] * Bv[k]; }
                if (!(rx * rx + ry * ry <= lim)) a.kept[i] = 0;
            }
        }
        if (fabs(coef[0]) < __builtin_huge_val()) {
            const double hy = 0.5 * (double)a.ny, hx = 0.5 * (double)a.nx;
            const double det = (coef[1] / hx) * (coef[8] / hy) - (coef[2] / hy) * (coef[7] / hx);
            if (!(0.5 <= det && det <= 2.0)) flags |= 8;
        }
    }
    if (tid == 0) {
        for (int k = 0; k < 12; k++) a.coef[k] = coef[k];
        a.stats[0] = n_used; a.stats[1] = rms_x; a.stats[2] = rms_y; a.stats[3] = (double)flags;
    }
}

__global__ __launch_bounds__(FIT_BLOCK) void k_align_fit(fit_args a, int poldeg) {
    __shared__ double s_red[FIT_WAVES];
    if (poldeg == 2) fit_body<6>(a, s_red);
    else fit_body<3>(a, s_red);
}

extern "C" int bbx_align_fit(bbx_ctx* ctx, int n_a, const int32_t* d_a_ys, const int32_t* d_a_xs, const float* d_a_off, const float* d_a_flux,
                             const float* d_a_err, int n_b, const int32_t* d_b_ys, const int32_t* d_b_xs, const float* d_b_off,
                             const float* d_b_flux, const float* d_b_err, int n_items, const int32_t* d_items, int ny, int nx, int poldeg,
                             float snr_min, double clip, int nmin, double* d_coef, double* d_stats, uint8_t* d_kept, void* stream) {
    if (!ctx || n_a < 0 || n_b < 0 || n_items < 0 || ny < 1 || nx < 1 || (poldeg != 1 && poldeg != 2) || !(clip > 0.0) || nmin < 0)
        return BBX_ERR_ARG;
    if (!d_coef || !d_stats || (n_items > 0 && (!d_items || !d_kept))) return BBX_ERR_ARG;
    if (n_a > 0 && (!d_a_ys || !d_a_xs || !d_a_off || !d_a_flux || !d_a_err)) return BBX_ERR_ARG;
    if (n_b > 0 && (!d_b_ys || !d_b_xs || !d_b_off || !d_b_flux || !d_b_err)) return BBX_ERR_ARG;
    fit_args a;
    a.A = {d_a_ys, d_a_xs, d_a_off, d_a_flux, d_a_err, n_a}; a.B = {d_b_ys, d_b_xs, d_b_off, d_b_flux, d_b_err, n_b};
    a.items = d_items; a.N = n_items; a.ny = ny; a.nx = nx; a.nmin = nmin; a.snr_min = snr_min; a.clip = clip;
    a.coef = d_coef; a.stats = d_stats; a.kept = d_kept;
    hipLaunchKernelGGL(k_align_fit, dim3(1), dim3(FIT_BLOCK), 0, (hipStream_t)stream, a, poldeg);
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// apply: a list through the inverse of T
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_align_apply(int n, const int32_t* __restrict__ ys, const int32_t* __restrict__ xs,
                                                     const float* __restrict__ off, const double* __restrict__ coef, int ny, int nx, int poldeg,
                                                     int32_t* __restrict__ oys, int32_t* __restrict__ oxs, float* __restrict__ ooff) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double c[6], d[6];
    for (int k = 0; k < 6; k++) { c[k] = coef[k]; d[k] = coef[6 + k]; }
    const double X = (double)xs[i] + (double)off[2 * (size_t)i + 1], Y = (double)ys[i] + (double)off[2 * (size_t)i];
    const double det = c[1] * d[2] - c[2] * d[1];
    double u = ((X - c[0]) * d[2] - c[2] * (Y - d[0])) / det;
    double v = (c[1] * (Y - d[0]) - (X - c[0]) * d[1]) / det;
    if (poldeg == 2)
        for (int it = 0; it < 2; it++) {
            const double bb[6] = {1.0, u, v, u * u, u * v, v * v};
            double fx = -X, fy = -Y;
            for (int k = 0; k < 6; k++) { fx = fx + c[k] * bb[k]; fy = fy + d[k] * bb[k]; }
            const double jxu = c[1] + 2.0 * c[3] * u + c[4] * v, jxv = c[2] + c[4] * u + 2.0 * c[5] * v;
            const double jyu = d[1] + 2.0 * d[3] * u + d[4] * v, jyv = d[2] + d[4] * u + 2.0 * d[5] * v;
            const double dj = jxu * jyv - jxv * jyu;
            const double un = u - (fx * jyv - jxv * fy) / dj, vn = v - (jxu * fy - fx * jyu) / dj;
            u = un; v = vn;
        }
    const double hy = 0.5 * (double)ny, hx = 0.5 * (double)nx;
    const double x = hx + hx * u, y = hy + hy * v;
    const bool ok = fabs(x) < 1e9 && fabs(y) < 1e9;                  // (false for NaN)
    const float nanf_ = __builtin_nanf("");
    if (ok) {
        const double fx = floor(x + 0.5), fy = floor(y + 0.5);
        oys[i] = (int32_t)fy; oxs[i] = (int32_t)fx;
        ooff[2 * (size_t)i] = (float)(y - fy); ooff[2 * (size_t)i + 1] = (float)(x - fx);
    } else {
        oys[i] = ys[i]; oxs[i] = xs[i];
        ooff[2 * (size_t)i] = nanf_; ooff[2 * (size_t)i + 1] = nanf_;
    }
}

extern "C" int bbx_align_apply(bbx_ctx* ctx, int n, const int32_t* d_ys, const int32_t* d_xs, const float* d_off, const double* d_coef, int ny,
                               int nx, int poldeg, int32_t* d_oys, int32_t* d_oxs, float* d_ooff, void* stream) {
    if (!ctx || n < 0 || ny < 1 || nx < 1 || (poldeg != 1 && poldeg != 2)) return BBX_ERR_ARG;
    if (n == 0) return BBX_OK;
    if (!d_ys || !d_xs || !d_off || !d_coef || !d_oys || !d_oxs || !d_ooff) return BBX_ERR_ARG;
    hipLaunchKernelGGL(k_align_apply, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, d_ys, d_xs, d_off, d_coef, ny, nx, poldeg,
                       d_oys, d_oxs, d_ooff);
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// grid: T at the lattice nodes
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_align_grid(const double* __restrict__ coef, int ny, int nx, int step, int gny, int gnx,
                                                    double* __restrict__ grid) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= gny * gnx) return;
    const int gj = k / gnx, gi = k - gj * gnx;
    const double hy = 0.5 * (double)ny, hx = 0.5 * (double)nx;
    const double u = ((double)gi * (double)step - hx) / hx, v = ((double)gj * (double)step - hy) / hy;
    const double b[6] = {1.0, u, v, u * u, u * v, v * v};
    double x = 0.0, y = 0.0;
    for (int t = 0; t < 6; t++) { x += b[t] * coef[t]; y += b[t] * coef[6 + t]; }
    grid[2 * (size_t)k] = x; grid[2 * (size_t)k + 1] = y;
}

extern "C" int bbx_align_grid(bbx_ctx* ctx, const double* d_coef, int ny, int nx, int step, int gny, int gnx, double* d_grid, void* stream) {
    if (!ctx || !d_coef || !d_grid || ny < 1 || nx < 1 || step < 1 || gny < 2 || gnx < 2 || (long long)gny * gnx > (1 << 24)) return BBX_ERR_ARG;
    // the lattice must hold the node after the last pixel in both directions (the resampler's condition)
    if ((ny - 1) / step + 1 >= gny || (nx - 1) / step + 1 >= gnx) return BBX_ERR_ARG;
    hipLaunchKernelGGL(k_align_grid, dim3((gny * gnx + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_coef, ny, nx, step, gny, gnx, d_grid);
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// the reference's mask on the new frame's grid
// ---------------------------------------------------------------------------------------------------------------------
struct rm_args {
    int in_ny, in_nx; const uint8_t* mask;
    int out_ny, out_nx; const double* grid; int gny, gnx, step;
    unsigned edge;
    uint8_t* out; unsigned long long* nedge;
};

// one output pixel: the lattice interpolation with the resampler's operations, the OR of the up-to-four input pixels, the
// edge bit where the 6 x 6 footprint leaves the input (or the position is not finite: every comparison is then false)
__device__ __forceinline__ unsigned rm_pixel(const rm_args& a, int X, int Y, bool* edge) {
    const int gj = Y / a.step, gi = X / a.step;                      // (gj + 1 < gny, gi + 1 < gnx: checked by the entry)
    const double fy = (double)(Y - gj * a.step) / (double)a.step, fx = (double)(X - gi * a.step) / (double)a.step;
    const double* g00 = a.grid + ((size_t)gj * a.gnx + gi) * 2;
    const double* g10 = g00 + (size_t)a.gnx * 2;
    double pos[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const double p = g00[k] + (g00[2 + k] - g00[k]) * fx;
        const double q = g10[k] + (g10[2 + k] - g10[k]) * fx;
        pos[k] = p + (q - p) * fy;
    }
    const double x = pos[0], y = pos[1];
    const double xf = floor(x), yf = floor(y);
    const bool inside = xf - 2.0 >= 0.0 && xf + 3.0 < (double)a.in_nx && yf - 2.0 >= 0.0 && yf + 3.0 < (double)a.in_ny;
    const bool near = xf >= -1.0 && xf < (double)a.in_nx && yf >= -1.0 && yf < (double)a.in_ny;
    unsigned v = 0;
    if (a.mask && near) {
        const int ix = (int)xf, iy = (int)yf;                        // -1 .. in - 1
        const bool px = x > xf, py = y > yf;                         // the pixel at + 1 only past the pixel centre
#pragma unroll
        for (int dy = 0; dy < 2; dy++)
#pragma unroll
            for (int dx = 0; dx < 2; dx++) {
                const int yy = iy + dy, xx = ix + dx;
                if ((dy == 0 || py) && (dx == 0 || px) && yy >= 0 && yy < a.in_ny && xx >= 0 && xx < a.in_nx)
                    v |= a.mask[(size_t)yy * a.in_nx + xx];
            }
    }
    *edge = !inside;
    return inside ? v : (v | a.edge);
}

__global__ __launch_bounds__(256) void k_remap_mask(rm_args a) {
    const size_t npix = (size_t)a.out_ny * a.out_nx;
    const size_t p0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    unsigned word = 0;
    int nedge = 0;
    if (p0 < npix) {
        int Y = (int)(p0 / a.out_nx), X = (int)(p0 - (size_t)Y * a.out_nx);
        const int nk = (int)min((size_t)4, npix - p0);
        for (int k = 0; k < nk; k++) {
            bool e;
            word |= (rm_pixel(a, X, Y, &e) & 255u) << (8 * k);
            nedge += e ? 1 : 0;
            if (++X == a.out_nx) { X = 0; Y++; }
        }
        if (nk == 4) *(uint32_t*)(a.out + p0) = word;                // (p0 is a multiple of 4; the entry checks the base)
        else for (int k = 0; k < nk; k++) a.out[p0 + k] = (uint8_t)(word >> (8 * k));
    }
    nedge = wave_sum_i32(nedge);                                     // (every lane of the wave is here)
    if ((threadIdx.x & 63) == 0 && nedge) atomicAdd(a.nedge, (unsigned long long)nedge);
}

extern "C" int bbx_remap_mask(bbx_ctx* ctx, int in_ny, int in_nx, const uint8_t* d_mask, int out_ny, int out_nx, const double* d_grid, int gny,
                              int gnx, int step, int edge_bit, uint8_t* d_out, int64_t* d_nedge, void* stream) {
    if (!ctx || !d_grid || !d_out || !d_nedge) return BBX_ERR_ARG;
    if (in_ny < 1 || in_nx < 1 || out_ny < 1 || out_nx < 1 || step < 1 || gny < 2 || gnx < 2 || edge_bit < 0 || edge_bit > 255) return BBX_ERR_ARG;
    if ((out_ny - 1) / step + 1 >= gny || (out_nx - 1) / step + 1 >= gnx) return BBX_ERR_ARG;
    if (((size_t)d_out & 3) != 0) return BBX_ERR_ARG;
    const size_t npix = (size_t)out_ny * out_nx;
    if ((npix + 1023) / 1024 > 0x7fffffffull) return BBX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    BBX_HIP(hipMemsetAsync(d_nedge, 0, sizeof(int64_t), s));
    rm_args a;
    a.in_ny = in_ny; a.in_nx = in_nx; a.mask = d_mask; a.out_ny = out_ny; a.out_nx = out_nx; a.grid = d_grid; a.gny = gny; a.gnx = gnx;
    a.step = step; a.edge = (unsigned)edge_bit; a.out = d_out; a.nedge = (unsigned long long*)d_nedge;
    hipLaunchKernelGGL(k_remap_mask, dim3((unsigned)((npix + 1023) / 1024)), dim3(256), 0, s, a);
    BBX_LAUNCH_CHECK();
    return BBX_OK;
}
