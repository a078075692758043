"""Fake stars: the definition.  A numpy restatement of bbx_fake_inject and bbx_fake_recover (include/bbx.h) with a
`dtype` argument, and the cases the host tests measure it on and the GPU tests (test_gpu_fake.py) compare the kernels with.

dtype is the arithmetic of what the kernel does in float32: the model's chain, the two passes of the shift, the square of sigma.  The
norm, A, q, the root F and everything added are float64 by definition; F is rounded to float32 where dtype is float32 (the kernel's
own F) and stays the float64 root otherwise.  The generator's integer stream is exact; its normal deviates are float64.
"""
import numpy as np
from scipy.optimize import brentq

import psfphot_ref as P

F32 = np.float32
MASKED, ON_SOURCE, OFF_FRAME, NO_PSF, NO_FLUX = 1, 2, 4, 8, 16

# largest distance of the float32 restatement from the float64 one over CASES (every group of every case), measured by
# test_fake_host.test_float32_follows_float64 (CPU, numpy), each rounded up in its last digit:
#   D32_F     |F32 / F64 - 1|                                  : 6.10e-8 (the rounding of F itself is up to 6e-8)
#   D32_ADD   |add32 - add64| / (F max P) over the stamp pixels: 1.88e-7
#   D32_NOISE noise on: |n32 - n64| / sqrt(F max P), n = sqrt(F max(P, 0)) g, the part of the add the deviates bring: 1.83e-7
# The GPU tests take 4 x these, the project's convention (the device adds its float64 sums in another, equally valid order).
D32_F = 6.2e-8
D32_ADD = 1.9e-7
D32_NOISE = 1.9e-7
# Candidates of a frame without fake stars that lie farther than a stamp from every star, looked up in the frame with them
# (test_gpu_fake.py, the scene of test_psfbuild_host.py).  They cannot keep their bits: the float32 transforms of a sub-image see other
# input and round differently everywhere.  Largest changes measured on an MI355X: |Scorr' - Scorr| 2.86e-6, |Fpsf' - Fpsf| / Fpsferr
# 3.04e-6, |Fpsferr' / Fpsferr - 1| 1.41e-7.  The test takes 4 x the figures below.
FAR_DSCORR, FAR_DFPSF, FAR_DFPSFERR = 2.9e-6, 3.1e-6, 1.5e-7
# noise on, a flat PSF on a zero frame with sigma 1: |(out - F P) / sqrt(F P) - g| of the float32 frame against the float64 deviate.
# out = fl32(F P + sqrt(F P) g): its rounding is 2^-24 |out|, divided by sqrt(F P).  With F P = 4 (the test's) and |g| < 6.7 (the
# largest deviate 2^-33 allows) |out| < 17.4, so the bound is 2^-24 17.4 / 2 = 5.2e-7; measured on the CPU restatement: 2.4e-7.
# The device's log and cos may differ from numpy's by a few ulp of float64: nothing next to it.
NOISE_TOL = 5.2e-7


# ---- the generator ----------------------------------------------------------------------------------------------------------
def philox4x32(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays of counters (uint32) with one key -> four uint32 arrays"""
    c = [np.asarray(v, np.uint64) & np.uint64(0xffffffff) for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0 & 0xffffffff), np.uint64(k1 & 0xffffffff)
    m32 = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return [v.astype(np.uint32) for v in c]


def star_words(seed, star, npx):
    """the integer stream of one star: words r0, r1 of the pixels 0 .. npx - 1"""
    seed = int(seed) & 0xffffffffffffffff
    r = philox4x32(np.arange(npx, dtype=np.uint64), np.uint64(star), 0, 0, seed & 0xffffffff, seed >> 32)
    return r[0], r[1]


def normals(seed, star, npx):
    """g_i of include/bbx.h: Box-Muller on (r0 + 0.5) / 2^32, (r1 + 0.5) / 2^32, float64"""
    r0, r1 = star_words(seed, star, npx)
    u1, u2 = (r0.astype(np.float64) + 0.5) / 4294967296.0, (r1.astype(np.float64) + 0.5) / 4294967296.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


# ---- S/N(F) and its root ----------------------------------------------------------------------------------------------------
def snr(Fl, p, v):
    """S/N(F) = F sqrt(sum p^2 / (v + F max(p, 0))), float64"""
    p, v = np.asarray(p, np.float64).ravel(), np.asarray(v, np.float64).ravel()
    return float(Fl * np.sqrt(np.sum(p * p / (v + Fl * np.maximum(p, 0.0)))))


def brackets(s, p, v):
    p, v = np.asarray(p, np.float64).ravel(), np.asarray(v, np.float64).ravel()
    A, q = float(np.sum(p * p / v)), float(np.max(np.maximum(p, 0.0) / v))
    s2 = float(s) * float(s)
    return float(s) / np.sqrt(A), (s2 * q + np.sqrt(s2 * s2 * q * q + 4.0 * A * s2)) / (2.0 * A), A, q


def flux_root(s, p, v):
    """F with S/N(F) = s, between the brackets"""
    lo, hi, _, _ = brackets(s, p, v)
    if not hi > lo or snr(lo, p, v) >= float(s):
        return lo
    if snr(hi, p, v) <= float(s):                                        # (a flat stamp under flat noise: the bracket is the root)
        return hi
    return brentq(lambda f: snr(f, p, v) - float(s), lo, hi, xtol=1e-300, rtol=4 * np.finfo(np.float64).eps, maxiter=500)


# ---- bbx_fake_inject --------------------------------------------------------------------------------------------------------
def stamp(cube, terms, idx, s, off, dtype):
    """steps 1-3 of bbx_psf_optflux_shift -> (P [S, S] in dtype, norm float64)"""
    cube = np.asarray(cube, F32)
    nplane, S = cube.shape[0], cube.shape[1]
    if terms is not None:
        Pm = P.model_chain(np.asarray(terms, F32)[s], cube, dtype).reshape(S, S)
    else:
        Pm = cube[min(max(int(idx[s]), 0), nplane - 1)].astype(dtype)
    dy, dx = F32(off[s][0]), F32(off[s][1])
    if not (abs(dy) <= 0.5 and abs(dx) <= 0.5):
        return Pm, float('nan')
    Pm = P.shift_stamp(Pm, dy, dx, dtype)
    with np.errstate(all='ignore'):
        return Pm, float(Pm.astype(np.float64).sum())


def inject_ref(frame, ref, sigma, mask_new, mask_ref, cube, terms, idx, ys, xs, off, s2n, clear_half=3, clear_nsigma=5.0, noise=False,
               seed=0, dtype=np.float64, star0=0):
    """bbx_fake_inject on a copy of frame (float32 [ny, nx]); sigma: a frame (the tests make it of a mini image where the kernel reads
    one).  star0: the index of the first star in its launch is 0; a caller that restates one launch star by star passes the star's.
    -> dict(out float32 frame, flux, real, snr_sky float64 [n] (rounded to float32 where dtype is float32), flags uint8 [n],
    add: per star None or the float64 [S, S] array of what was added, pmax: per star max P)"""
    t = dtype
    out = np.array(frame, F32)
    sigma = np.asarray(sigma, F32)
    ny, nx = out.shape
    S = np.asarray(cube).shape[1]
    h, n = S // 2, len(ys)
    off = np.asarray(off, F32).reshape(n, 2)
    flux, real, snr_sky, flags = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n, np.uint8)
    adds, pmax = [None] * n, np.zeros(n)
    nsig = F32(clear_nsigma)
    for s in range(n):
        Pm, norm = stamp(cube, terms, idx, s, off, t)
        if not (norm > 0 and norm < 1e300):
            flags[s] = NO_PSF
            continue
        y, x = int(ys[s]), int(xs[s])
        y0, x0 = y - h, x - h
        if y0 < 0 or x0 < 0 or y0 + S > ny or x0 + S > nx:
            flags[s] = OFF_FRAME
            continue
        ya, yb, xa, xb = max(y - clear_half, 0), min(y + clear_half + 1, ny), max(x - clear_half, 0), min(x + clear_half + 1, nx)
        if (mask_new is not None and mask_new[ya:yb, xa:xb].any()) or (mask_ref is not None and mask_ref[ya:yb, xa:xb].any()):
            flags[s] = MASKED
            continue
        with np.errstate(all='ignore'):
            lim = nsig * sigma[ya:yb, xa:xb]                             # float32
            w = out[ya:yb, xa:xb]
            hit = (~np.isfinite(w) | (np.abs(w) > lim)).any()
            if ref is not None:
                r = np.asarray(ref, F32)[ya:yb, xa:xb]
                hit = hit or (~np.isfinite(r) | (np.abs(r) > lim)).any()
        if hit:
            flags[s] = ON_SOURCE
            continue
        sg = sigma[y0:y0 + S, x0:x0 + S].astype(t)
        sn = F32(s2n[s])
        with np.errstate(all='ignore'):
            v = (sg * sg).astype(np.float64)
            if not (sn > 0 and np.isfinite(sn)) or not (np.isfinite(sg) & (sg > 0) & (v > 0)).all():
                flags[s] = NO_FLUX
                continue
        p = Pm.astype(np.float64) / norm
        _, _, A, q = brackets(float(sn), p, v)
        if not (A > 0 and A < 1e300 and q < 1e300):
            flags[s] = NO_FLUX
            continue
        Fl = flux_root(float(sn), p, v)
        if t is np.float32:
            with np.errstate(over='ignore'):
                Fl = float(F32(Fl))
        if not (Fl > 0 and Fl < 3e38):
            flags[s] = NO_FLUX
            continue
        add = Fl * p
        if noise:
            add = add + np.sqrt(Fl * np.maximum(p, 0.0)) * normals(seed, star0 + s, S * S).reshape(S, S)
        out[y0:y0 + S, x0:x0 + S] = (out[y0:y0 + S, x0:x0 + S].astype(np.float64) + add).astype(F32)
        flux[s], real[s], snr_sky[s] = Fl, float(add.sum()), Fl * np.sqrt(A)
        adds[s], pmax[s] = add, float(p.max())
    if t is np.float32:
        flux, real, snr_sky = (a.astype(F32).astype(np.float64) for a in (flux, real, snr_sky))
    return dict(out=out, flux=flux, real=real, snr_sky=snr_sky, flags=flags, add=adds, pmax=pmax)


# ---- bbx_fake_recover -------------------------------------------------------------------------------------------------------
def recover_ref(scorr, fpsf, fpsferr, ys, xs, radius):
    """-> float32 [n, 6]"""
    scorr, fpsf, fpsferr = (np.asarray(a, F32) for a in (scorr, fpsf, fpsferr))
    ny, nx = scorr.shape
    out = np.zeros((len(ys), 6), F32)
    for s, (y, x) in enumerate(zip(np.asarray(ys).tolist(), np.asarray(xs).tolist())):
        ya, yb, xa, xb = max(y - radius, 0), min(y + radius + 1, ny), max(x - radius, 0), min(x + radius + 1, nx)
        w = scorr[ya:yb, xa:xb] if ya < yb and xa < xb else np.zeros((0, 0), F32)
        fin = np.isfinite(w)
        if not fin.any():
            out[s, :2] = np.nan
            continue
        k = int(np.argmax(np.where(fin, w, -np.inf)))                    # the first of equal values in row-major order
        r, c = divmod(k, w.shape[1])
        at = fpsf[y, x] if 0 <= y < ny and 0 <= x < nx else 0.0
        out[s] = (ya + r - y, xa + c - x, w[r, c], fpsf[ya + r, xa + c], fpsferr[ya + r, xa + c], at)
    return out


# ---- the cases of the kernel tests ------------------------------------------------------------------------------------------
BOX, SKY, CLEAR_HALF, CLEAR_NSIGMA = 16, 10.0, 3, 5.0
NPLANE_TERMS, NPLANE_IDX = 6, 12
# (ny, nx, S, PSF form, sigma form: 'frame', 'mini_x' (interp_Xchan True), 'mini_c' (False)); a mini image needs a frame of whole boxes
CASES = ((96, 128, 9, 'terms', 'frame'), (96, 128, 9, 'idx', 'mini_x'), (96, 128, 25, 'idx', 'mini_c'), (96, 128, 25, 'terms', 'mini_x'),
         (96, 128, 49, 'terms', 'mini_c'), (96, 128, 49, 'idx', 'frame'), (101, 131, 9, 'idx', 'frame'), (101, 131, 25, 'terms', 'frame'),
         (101, 131, 49, 'idx', 'frame'))


def wing_stamp(S, fwhm, dy=0.0, dx=0.0):
    """a Moffat stamp with small negative wings (what a PSFEx model's outskirts look like): the profile minus its value in the
    middle of the stamp's first row, so that the corners lie below zero"""
    p = P.moffat_stamp(S, fwhm, dy, dx)
    p = p - p[0, S // 2]
    return p / p.sum()


def make_stars(ny, nx, S):
    """the stars of a case -> list of dict(y, x, off, s2n, tag, want: the flag its features ask for, feats: what is planted for it,
    (kind, y, x))"""
    h, ch = S // 2, CLEAR_HALF
    cy, cx = ny // 2, nx // 2
    st = []

    def add(tag, y, x, off=(0.0, 0.0), s2n=20.0, want=0, feats=()):
        st.append(dict(tag=tag, y=y, x=x, off=off, s2n=s2n, want=want, feats=tuple(feats)))
    add('centre', cy, cx)
    add('corner_tl', h, h, (0.5, -0.5), 5.0)
    add('touching', h, h + S, (0.25, -0.125), 50.0)                     # Chebyshev distance exactly S from corner_tl
    add('corner_br', ny - 1 - h, nx - 1 - h, (-0.5, 0.5), 5.0)
    add('corner_tr', h, nx - 1 - h, (0.0, 0.5), 7.0)
    add('corner_bl', ny - 1 - h, h, (-0.5, 0.0), 7.0)
    for tag, y, x in (('off_top', h - 1, cx), ('off_bottom', ny - h, cx), ('off_left', cy, h - 1), ('off_right', cy, nx - h),
                      ('off_corner', h - 1, h - 1)):
        add(tag, y, x, want=OFF_FRAME)
    add('mask_new_edge', cy, cx, want=MASKED, feats=[('mask_new', cy + ch, cx - ch)])
    add('mask_new_out', cy, cx, feats=[('mask_new', cy + ch + 1, cx)])
    add('mask_ref_edge', cy, cx, want=MASKED, feats=[('mask_ref', cy - ch, cx + ch)])
    add('mask_ref_out', cy, cx, feats=[('mask_ref', cy, cx - ch - 1)])
    add('bright_new', cy, cx, want=ON_SOURCE, feats=[('bright_new', cy + 1, cx - 2)])
    add('bright_ref', cy, cx, want=ON_SOURCE, feats=[('bright_ref', cy - ch, cx)])
    add('nan_new', cy, cx, want=ON_SOURCE, feats=[('nan_new', cy, cx + ch)])
    add('no_psf', cy, cx, want=NO_PSF)
    add('s2n_zero', cy, cx, s2n=0.0, want=NO_FLUX)
    add('s2n_neg', cy, cx, s2n=-3.0, want=NO_FLUX)
    add('s2n_nan', cy, cx, s2n=np.nan, want=NO_FLUX)
    add('sigma_zero', cy, cx, want=NO_FLUX, feats=[('sigma_zero', cy + h, cx + h)])       # (sigma frames only)
    add('s2n_tiny', cy, cx, (0.3, 0.2), 1e-3)
    add('s2n_huge', cy, cx, (-0.2, 0.4), 1e4)
    return st


def make_groups(stars, S):
    """the launches of a case: a star joins the first group whose stars are all at least S away (Chebyshev).  A planted feature lies
    within its own star's stamp, so it meets the star it was planted for and no other of the group"""
    groups = []
    for s in stars:
        for g in groups:
            if all(max(abs(s['y'] - o['y']), abs(s['x'] - o['x'])) >= S for o in g):
                g.append(s)
                break
        else:
            groups.append([s])
    return groups


def make_case(ny, nx, S, form, sig_form, seed=5):
    """-> dict(frame, ref, mini (sigma mini image; None for a frame that is no whole number of boxes), sigma (the frame), cube, groups:
    list of dict(stars, frame, ref, sigma, mask_new, mask_ref, terms, idx, ys, xs, off, s2n))"""
    rs = np.random.RandomState(seed + 3 * S + ny)
    mini = channels = None
    if ny % BOX == 0 and nx % BOX == 0:
        by, bx = np.mgrid[0:ny // BOX, 0:nx // BOX]
        mini = (SKY + 1.5 * np.sin(by / 2.0) * np.cos(bx / 3.0) + 0.3 * rs.random_sample(by.shape) + 0.5 * (by // 3)).astype(F32)
        import zogy_core as Z
        if sig_form == 'mini_c':
            from blackbox_amd import settings
            channels = (mini.shape[0] // settings.ny, mini.shape[1] // settings.nx)
        sigma = np.asarray(Z.mini2back(mini, (ny, nx), BOX, channels=channels), F32)
    else:
        gy, gx = np.mgrid[0:ny, 0:nx]
        sigma = (SKY + 1.5 * np.sin(gy / 30.0) * np.cos(gx / 40.0)).astype(F32)
    frame = (rs.normal(0, 1, (ny, nx)) * sigma).astype(F32)
    ref = (rs.normal(0, 1, (ny, nx)) * sigma * 0.5).astype(F32)
    frame, ref = np.clip(frame, -4.5 * sigma, 4.5 * sigma), np.clip(ref, -4.5 * sigma, 4.5 * sigma)     # (no chance source in a window)
    if form == 'idx':
        cube = np.stack([wing_stamp(S, 3.0 + 0.1 * q) for q in range(NPLANE_IDX - 1)] + [np.zeros((S, S))]).astype(F32)
    else:
        base = wing_stamp(S, 3.4)
        cube = np.stack([base] + [0.05 * (wing_stamp(S, 3.0 + 0.15 * q) - base) for q in range(1, NPLANE_TERMS)]).astype(F32)
    groups = []
    for g in make_groups(make_stars(ny, nx, S), S):
        if sig_form != 'frame' and any(f[0] == 'sigma_zero' for s in g for f in s['feats']):
            continue                                                     # (a mini image has no single pixel to set)
        a = dict(frame=frame.copy(), ref=ref.copy(), sigma=sigma.copy(), mask_new=np.zeros((ny, nx), np.uint8), mask_ref=np.zeros((ny, nx), np.uint8))
        for s in g:
            for kind, y, x in s['feats']:
                if kind in ('mask_new', 'mask_ref'):
                    a[kind][y, x] = 4
                elif kind == 'sigma_zero':
                    a['sigma'][y, x] = 0.0
                else:
                    a['frame' if kind.endswith('new') else 'ref'][y, x] = np.nan if kind.startswith('nan') else 5.5 * sigma[y, x]
        ys, xs = np.array([s['y'] for s in g], np.int32), np.array([s['x'] for s in g], np.int32)
        terms = idx = None
        if form == 'idx':
            idx = np.array([NPLANE_IDX - 1 if s['tag'] == 'no_psf' else (3 * k + s['y']) % (NPLANE_IDX - 1) for k, s in enumerate(g)], np.int32)
        else:
            from blackbox_amd import zogy as G
            terms = G.psf_poly_terms(xs + 1.0, ys + 1.0, ((nx + 1) / 2.0, (ny + 1) / 2.0), (nx / 2.0, ny / 2.0), 2)
            for k, s in enumerate(g):
                if s['tag'] == 'no_psf':
                    terms[k] = 0
        a.update(stars=g, ys=ys, xs=xs, terms=terms, idx=idx, off=np.array([s['off'] for s in g], F32).reshape(-1, 2),
                 s2n=np.array([s['s2n'] for s in g], F32))
        groups.append(a)
    return dict(ny=ny, nx=nx, S=S, form=form, sig_form=sig_form, mini=mini, cube=cube, groups=groups)


def run_group(case, g, dtype=np.float64, noise=False, seed=0):
    return inject_ref(g['frame'], g['ref'], g['sigma'], g['mask_new'], g['mask_ref'], case['cube'], g['terms'], g['idx'], g['ys'], g['xs'],
                      g['off'], g['s2n'], CLEAR_HALF, CLEAR_NSIGMA, noise, seed, dtype)
