"""Transient vetting: the definition.  A numpy restatement of bbx_zogy_pd_stamps and bbx_trans_psffit (include/bbx.h)
with a `dtype` argument, and the cases the host tests (test_transfit_host.py) measure it on and the GPU tests
(test_gpu_transfit.py) compare the kernels with.

bbx_zogy_pd_stamps works in float64 throughout and rounds its stamp to float32 at the end: its restatement is numpy.fft on the
same M x M grid; dtype only says whether the stamp is returned rounded.

bbx_trans_psffit: dtype is the arithmetic of what the kernel does in float32 -- the two passes of the shift and V_D.  theta, the
taps and their split are float32 by definition; the norm, the sums and the 3 x 3 solve are float64 by definition.  dtype = float64
is the value the kernel approximates; dtype = float32 follows it operation by operation (but for the order of the float64 sums)
and rounds the five outputs to float32.
"""
import numpy as np

import psfphot_ref as PR

F = np.float32
AT_BOUND, MASKED, NO_FIT, NOT_CONVERGED = 1, 2, 4, 8
STEP_MAX, STEP_TOL = 0.5, 0.01

# ---- measured constants (CPU, numpy), each by the test named; the GPU tests allow 4 x the D32_* for the device's summation order,
# the margin psfphot_ref.TOL uses.
# pytest tests/test_transfit_host.py -k float32_follows_float64 -s
#   largest |x32 / x64 - 1| of flux, err, chi2 and largest |x32 - x64| of dy, dx [pixel] over CASES: 2.07e-7, 2.51e-7, 1.11e-5
#   (a chi2 of 0.02 on one degree of freedom under W = 3), 6.18e-7 px
D32_FLUX, D32_ERR, D32_CHI2, D32_POS = 2.1e-7, 2.6e-7, 1.2e-5, 6.5e-7
# pytest tests/test_transfit_host.py -k pd_on_the_small_grid -s
#   largest |P_D(M = 256) - P_D(L = 1400)| / peak over the Moffat pairs of PD_PAIRS at S = 49: 4.3e-16 (a stamp of 49 pixels embedded
#   in either grid has the same samples of the same band-limited spectrum); largest fold of those pairs: 1.02e-4 (FWHM 4.6 / 3.3);
#   fold of a point (new) / 5 x 5 box (reference) pair under a deep reference, sigma_n / sigma_r = 50: 0.147 (at sigma_n /
#   sigma_r = 2 the new image's noise term keeps the denominator smooth and the pair folds 7e-6)
PD_GRID_DEV, PD_FOLD_MOFFAT, PD_FOLD_BOX = 1e-15, 1.1e-4, 0.14
PD_FOLD_WARN = 0.01                                                  # zogy.PD_FOLD_WARN: 90 x the first, 1 / 14 of the second
# the kernel's P_D against this restatement: both work in float64; what remains is the float32 rounding of the stamp (6e-8 of a
# pixel's own value) and the order of four passes of <= 512 float64 terms (1e-13): 2e-7 of the peak bounds both
PD_TOL = 2e-7
# fold is a ratio of two float64 sums rounded to float32
FOLD_TOL = 2e-7


# ---- P_D --------------------------------------------------------------------------------------------------------------------
def embed(P, M):
    """the stamp on an M x M grid, its centre on the origin"""
    S = P.shape[0]
    h = S // 2
    g = np.zeros((M, M))
    i = (np.arange(S) - h) % M
    g[np.ix_(i, i)] = np.asarray(P, np.float64)
    return g


def pd_grid(pn, pr, sc, M):
    """p[M][M] float64 of one sub-image: oracle/zogy_core.run_zogy's PDh on the M grid, back in real space"""
    sn, sr, fn, fr = (np.float64(F(v)) for v in sc[:4])
    Pnh, Prh = np.fft.fft2(embed(pn, M)), np.fft.fft2(embed(pr, M))
    Pn2, Pr2 = Pnh.real ** 2 + Pnh.imag ** 2, Prh.real ** 2 + Prh.imag ** 2
    sn2, sr2, fn2, fr2 = sn * sn, sr * sr, fn * fn, fr * fr
    fD = fr * fn / np.sqrt(sn2 * fr2 + sr2 * fn2)
    den = (sn2 * fr2) * Pr2 + (sr2 * fn2) * Pn2
    with np.errstate(all='ignore'):
        PDh = np.where(den > 0, ((fr * fn) / fD) * (Prh * Pnh) / np.sqrt(np.where(den > 0, den, 1.0)), 0.0)
    return np.fft.ifft2(PDh).real


def positive(v):
    return bool(np.isfinite(v) and v > 0)


def pd_stamps_ref(pn, pr, scal, M, dtype=np.float64):
    """bbx_zogy_pd_stamps.  pn, pr float32 [nsub, S, S], scal [nsub, 6] -> (pd [nsub, S, S], fold [nsub]); float32 where dtype is"""
    pn, pr = np.asarray(pn, F), np.asarray(pr, F)
    nsub, S = pn.shape[0], pn.shape[1]
    h = S // 2
    pd, fold = np.zeros((nsub, S, S)), np.ones(nsub)
    i = (np.arange(S) - h) % M
    for k in range(nsub):
        sc = np.asarray(scal[k], F)
        with np.errstate(all='ignore'):
            live = all(positive(v) for v in sc[:4]) and positive(pn[k].astype(np.float64).sum()) and positive(pr[k].astype(np.float64).sum())
            if not live:
                continue
            p = pd_grid(pn[k], pr[k], sc, M)
        st = p[np.ix_(i, i)]
        tot, ins, sm = np.abs(p).sum(), np.abs(st).sum(), st.sum()
        if not (positive(sm) and positive(tot)):
            continue
        pd[k], fold[k] = st / sm, (tot - ins) / tot
    if dtype is np.float32:
        return pd.astype(F), fold.astype(F)
    return pd, fold


# ---- the fit ----------------------------------------------------------------------------------------------------------------
def variance_d(N, R, sig_n, sig_r, fn, fr, dtype):
    """V_D = (fr^2 Vn + fn^2 Vr) / (fr fn)^2, Vn = max(N, 0) + sigma_n^2 (bbx_variance's: fmaxf, a NaN N counts 0), in dtype, operation
    by operation"""
    t = dtype
    fn, fr = t(F(fn)), t(F(fr))
    with np.errstate(all='ignore'):
        vn = np.fmax(N.astype(t), t(0)) + sig_n.astype(t) * sig_n.astype(t)
        vr = np.fmax(R.astype(t), t(0)) + sig_r.astype(t) * sig_r.astype(t)
        ff = fr * fn
        return ((fr * fr) * vn + (fn * fn) * vr) / (ff * ff)


def solve3(m, r):
    """the symmetric 3 x 3 system by cofactors, in the kernel's order -> (F, a, b) or None (det zero or not finite)"""
    m00, m01, m02, m11, m12, m22 = m
    r0, r1, r2 = r
    with np.errstate(all='ignore'):
        c00, c01, c02 = m11 * m22 - m12 * m12, m02 * m12 - m01 * m22, m01 * m12 - m02 * m11
        det = (m00 * c00 + m01 * c01) + m02 * c02
        if not (det != 0 and abs(det) <= 1e300):
            return None
        c11, c12, c22 = m00 * m22 - m02 * m02, m01 * m02 - m00 * m12, m00 * m11 - m01 * m01
        return (((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det, ((c02 * r0 + c12 * r1) + c22 * r2) / det,
                (c11 / det, c22 / det))


def fin(v):
    return bool(abs(v) <= 1e300)


def trans_psffit_ref(D, N, R, sig_n, sig_r, mask, pd, ys, xs, scal, size, nsx, W=11, niter=8, maxshift=2.0, dtype=np.float64):
    """bbx_trans_psffit.  D, N, R, sig_n, sig_r [ny, nx] float32 (the sigma maps: frames; the tests make them of mini images where the
    kernel reads those), mask uint8 or None, pd float32 [nsub, S, S] -> dict(flux, err, dy, dx, chi2 float64 [n] (rounded to float32
    where dtype is float32), flags uint8 [n]; and what the kernel does not write: last [n], the last unclamped step (NaN: none),
    dy_err, dx_err [n], the position errors of the last solve)"""
    t = dtype
    D, N, R, sig_n, sig_r = (np.asarray(a, F) for a in (D, N, R, sig_n, sig_r))
    ny, nx = D.shape
    pd = np.asarray(pd, F)
    nsub, S = pd.shape[0], pd.shape[1]
    nsy = nsub // nsx
    h, hw = S // 2, W // 2
    n = len(ys)
    out = {k: np.zeros(n) for k in ('flux', 'err', 'dy', 'dx', 'chi2', 'dy_err', 'dx_err')}
    out['last'] = np.full(n, np.nan)
    flags = np.zeros(n, np.uint8)
    bound = np.float64(F(maxshift))
    for c in range(n):
        y0, x0 = int(ys[c]), int(xs[c])
        if y0 < 0 or y0 >= ny or x0 < 0 or x0 >= nx:
            flags[c] = NO_FIT
            continue
        k = min(y0 // size, nsy - 1) * nsx + min(x0 // size, nsx - 1)
        fn, fr = scal[k][2], scal[k][3]
        ya, yb, xa, xb = max(y0 - hw, 0), min(y0 + hw + 1, ny), max(x0 - hw, 0), min(x0 + hw + 1, nx)
        wy, wx = np.mgrid[ya:yb, xa:xb]
        sy, sx = (wy - y0 + h).ravel(), (wx - x0 + h).ravel()           # stamp indices of the window's pixels on the frame
        d = D[ya:yb, xa:xb].ravel()
        use = np.ones(d.shape, bool)
        if mask is not None:
            hit = mask[ya:yb, xa:xb].ravel() != 0
            if hit.any():
                flags[c] |= MASKED
            use &= ~hit
        use &= np.isfinite(d)
        with np.errstate(all='ignore'):
            v = variance_d(N[ya:yb, xa:xb].ravel(), R[ya:yb, xa:xb].ravel(), sig_n[ya:yb, xa:xb].ravel(), sig_r[ya:yb, xa:xb].ravel(), fn, fr, t)
            use &= (v > 0) & np.isfinite(v)
        n_used = int(use.sum())
        if n_used < 4:
            flags[c] = (flags[c] & MASKED) | NO_FIT
            continue
        d, v, sy, sx = d[use].astype(np.float64), v[use].astype(np.float64), sy[use], sx[use]

        def place(ty, tx):
            P = PR.shift_stamp(pd[k], ty, tx, t)
            with np.errstate(all='ignore'):
                norm = float(P.astype(np.float64).sum())
            if not (norm > 0 and norm < 1e300):
                return None
            return P.astype(np.float64) / norm

        ty, tx = F(0), F(0)
        stopped = nofit = False
        last = 0.0
        perr = (0.0, 0.0)
        for _ in range(niter):
            P = place(ty, tx)
            if P is None:
                nofit = True
                break
            p = P[sy, sx]
            ux = -((P[sy, sx + 1] - P[sy, sx - 1]) / 2.0)
            uy = -((P[sy + 1, sx] - P[sy - 1, sx]) / 2.0)
            with np.errstate(all='ignore'):
                m = [float((a * b / v).sum()) for a, b in ((p, p), (p, ux), (p, uy), (ux, ux), (ux, uy), (uy, uy))]
                r = [float((a * d / v).sum()) for a in (p, ux, uy)]
                sol = solve3(m, r)
                if sol is None:
                    stopped = True
                    break
                Fl, ca, cb, cov = sol
                if not (Fl != 0 and fin(Fl)):
                    stopped = True
                    break
                ddy, ddx = cb / Fl, ca / Fl
                if not (fin(ddy) and fin(ddx)):
                    stopped = True
                    break
                perr = (np.sqrt(abs(cov[1])) / abs(Fl), np.sqrt(abs(cov[0])) / abs(Fl))
            last = max(abs(ddy), abs(ddx))
            ty = F(min(max(np.float64(ty) + min(max(ddy, -STEP_MAX), STEP_MAX), -bound), bound))
            tx = F(min(max(np.float64(tx) + min(max(ddx, -STEP_MAX), STEP_MAX), -bound), bound))
        if not nofit:
            P = place(ty, tx)
            nofit = P is None
        if not nofit:
            p = P[sy, sx]
            with np.errstate(all='ignore'):
                num, den = float((p * d / v).sum()), float((p * p / v).sum())
            nofit = not (den > 0 and fin(den) and fin(num))
        if nofit:
            flags[c] = (flags[c] & MASKED) | NO_FIT
            continue
        Fl = num / den
        e = d - Fl * p
        out['flux'][c], out['err'][c], out['dy'][c], out['dx'][c] = Fl, 1.0 / np.sqrt(den), ty, tx
        out['chi2'][c] = float((e * e / v).sum()) / (n_used - 3)
        out['last'][c] = np.inf if stopped else last
        out['dy_err'][c], out['dx_err'][c] = perr
        if abs(ty) >= F(maxshift) or abs(tx) >= F(maxshift):
            flags[c] |= AT_BOUND
        if stopped or last > STEP_TOL:
            flags[c] |= NOT_CONVERGED
    if t is np.float32:
        for k in ('flux', 'err', 'dy', 'dx', 'chi2'):
            with np.errstate(all='ignore'):
                out[k] = out[k].astype(F).astype(np.float64)
    out['flags'] = flags
    return out


# ---- the cases of the kernel tests --------------------------------------------------------------------------------------------
NY, NX, SIZE, NSY, NSX, BOX = PR.NY, PR.NX, PR.SIZE, PR.NSY, PR.NSX, PR.BOX
NSUB = NSY * NSX
NITER, MAXSHIFT = 8, 2.0
# (S, W, ncand, sigma form: 'frame', 'mini_x' (interp_Xchan True), 'mini_c' (False), mask: None, 'zero', 'hits')
CASES = ((15, 3, 1, 'frame', None), (15, 5, 65, 'mini_x', 'zero'), (21, 5, 300, 'mini_c', 'hits'), (21, 11, 65, 'frame', 'hits'),
         (49, 11, 300, 'mini_x', None), (49, 3, 65, 'mini_c', 'zero'), (49, 11, 1, 'frame', 'zero'), (21, 3, 300, 'frame', 'hits'))
FAR = 9                                                              # the candidate whose source lies 2.5 px from its peak
# pd_stamps: (S, M, nsub), the last sub-image dead where nsub > 1
PD_CASES = ((15, 64, 1), (15, 64, 12), (15, 256, 12), (21, 256, 1), (21, 256, 12), (49, 256, 1), (49, 256, 12))
# Moffat pairs (FWHM new, FWHM ref) [pixel] over the FWHM range of bench.py's scene (new 3.6 .. 4.6, reference 3.3 .. 3.9), equal and unequal
PD_PAIRS = ((3.6, 3.3), (4.6, 3.9), (3.6, 3.9), (4.6, 3.3), (3.6, 3.6), (3.9, 3.9))


def make_scal(seed=0):
    rs = np.random.RandomState(100 + seed)
    scal = np.zeros((NSUB, 6), F)
    scal[:, 0], scal[:, 1] = rs.uniform(9, 11, NSUB), rs.uniform(4, 6, NSUB)
    scal[:, 2], scal[:, 3] = 1.0, rs.uniform(0.8, 1.25, NSUB)
    scal[:, 4:] = 0.1
    return scal


def make_pd_case(S, M, nsub, seed=0):
    rs = np.random.RandomState(11 + S + nsub)
    pn = np.stack([PR.moffat_stamp(S, 3.0 + 0.1 * q, 0.1 * (q % 3), -0.07 * (q % 4)) for q in range(nsub)]).astype(F)
    pr = np.stack([PR.moffat_stamp(S, 4.0 - 0.07 * q) for q in range(nsub)]).astype(F)
    pn += (rs.normal(0, 2e-5, pn.shape)).astype(F)
    scal = make_scal(seed)[:nsub].copy()
    if nsub > 1:
        scal[nsub - 1, 1] = np.nan                                   # a dead tile
        scal[nsub // 2, 2] = 0.0                                     # ... and another
    return dict(pn=pn, pr=pr, scal=scal, M=M)


SPECIAL = ((0, 0), (0, NX - 1), (NY - 1, 0), (NY - 1, NX - 1), (0, NX // 2), (NY - 1, NX // 3), (NY // 2, 0), (NY // 3, NX - 1))
NEIGHBOUR = ((0, 1), (1, 0), (0, -1), (-1, 0), (1, 1), (-1, -1), (1, -1), (-1, 1))


def source_positions(rs):
    """the sources' integer positions: eight in the corners and on the edges (psfphot_ref's), the rest on a grid of 12 px in random
    order, so that no source's core lies in another's fit window"""
    gy, gx = np.mgrid[12:NY - 8:12, 12:NX - 4:12]
    cells = np.stack([gy.ravel(), gx.ravel()], axis=1).tolist()
    keep = [p for p in cells if all(max(abs(p[0] - s[0]), abs(p[1] - s[1])) >= 12 for s in SPECIAL)]
    return list(SPECIAL) + [tuple(keep[i]) for i in rs.permutation(len(keep))]


def make_case(S, W, ncand, sig_form, mask_form, seed=5):
    """-> dict(D, N, R, mini_n, mini_r, sig_form, mask, pd, scal, ys, xs, W, off, flux): point sources of P_D of either sign, S/N 100
    and up, on a frame of 96 x 128 with noise of V_D.  Candidate c < the number of sources: the source's own peak, the source at
    peak + off, |off| <= 0.5 (source FAR: 2.5 px); the candidates beyond walk round the sources' neighbouring pixels (clipped to the
    frame), so their sources lie up to 1.5 px from the peak.  The first eight peaks are in the corners and on the edges"""
    rs = np.random.RandomState(seed + 7 * S + ncand + W)
    src = source_positions(rs)
    ns = len(src)
    soff = rs.uniform(-0.5, 0.5, (ns, 2))
    soff[FAR] = (0.2, 2.5)
    sflux = 10 ** rs.uniform(4.0, 4.7, ns) * np.where(np.arange(ns) % 3 == 1, -1.0, 1.0)
    ys, xs, off, flux = [], [], [], []
    for c in range(ncand):
        j, ring = (c, None) if c < ns else ((c - ns) % ns, NEIGHBOUR[((c - ns) // ns) % 8])
        y, x = src[j]
        if ring is not None:
            y, x = min(max(y + ring[0], 0), NY - 1), min(max(x + ring[1], 0), NX - 1)
        ys.append(y); xs.append(x); flux.append(sflux[j])
        off.append((src[j][0] + soff[j][0] - y, src[j][1] + soff[j][1] - x))
    ys, xs, off, flux = np.array(ys, np.int32), np.array(xs, np.int32), np.array(off), np.array(flux)
    n = ncand
    scal = make_scal(seed)
    pd = np.stack([PR.moffat_stamp(S, 3.6 + 0.1 * q) for q in range(NSUB)]).astype(F)
    by, bx = np.mgrid[0:NY // BOX, 0:NX // BOX]
    mini_n = (10.0 + 1.5 * np.sin(by / 2.0) * np.cos(bx / 3.0) + 0.3 * rs.random_sample(by.shape) + 0.5 * (by // 3)).astype(F)
    mini_r = (5.0 + 0.5 * np.cos(by / 2.0) + 0.2 * rs.random_sample(by.shape)).astype(F)
    img = np.zeros((NY, NX))
    gy, gx = np.mgrid[0:NY, 0:NX]
    for (y, x), o, f in zip(src[:max(min(ns, ncand), 1)], soff, sflux):
        k = (y // SIZE) * NSX + x // SIZE
        ya, yb, xa, xb = max(y - 20, 0), min(y + 21, NY), max(x - 20, 0), min(x + 21, NX)
        img[ya:yb, xa:xb] += f * PR.moffat(3.6 + 0.1 * k, gy[ya:yb, xa:xb] - (y + o[0]), gx[ya:yb, xa:xb] - (x + o[1]))
    R = (np.abs(img) * 0.5 + rs.normal(0, 5.0, img.shape)).astype(F)
    N = (R + img + rs.normal(0, 10.0, img.shape)).astype(F)
    fr = scal[(gy // SIZE) * NSX + gx // SIZE, 3].astype(np.float64)
    vd = (fr ** 2 * (np.maximum(N, 0) + 100.0) + (np.maximum(R, 0) + 25.0)) / fr ** 2
    D = (img + rs.normal(0, 1, img.shape) * np.sqrt(vd)).astype(F)
    if n > 12:
        D[ys[12] + 1, xs[12]] = np.nan                               # a NaN in a window
        N[ys[11], xs[11] - 1] = np.nan                               # ... and one in the new frame: it counts 0 in Vn
    mask = None
    if mask_form == 'zero':
        mask = np.zeros((NY, NX), np.uint8)
    elif mask_form == 'hits':
        mask = (rs.random_sample((NY, NX)) < 0.002).astype(np.uint8) * rs.randint(1, 255, (NY, NX)).astype(np.uint8)
        mask[ys[0], xs[0]] = 4                                       # the first peak sits in a corner: W = 3 leaves it 3 pixels
        mask[min(ys[-1] + W // 2, NY - 1), xs[-1]] = 1               # ... and in the last window's outermost row
    return dict(D=D, N=N, R=R, mini_n=mini_n, mini_r=mini_r, sig_form=sig_form, mask=mask, pd=pd, scal=scal, ys=ys, xs=xs, W=W, off=off,
                flux=flux)


def sigma_frames(case):
    """the two sigma frames of a case: the oracle's zoom of its mini images (psfphot_ref.sigma_frame)"""
    return tuple(PR.sigma_frame(dict(mini=case[m], sig_form=case['sig_form'])) for m in ('mini_n', 'mini_r'))


def run_case(case, dtype=np.float64, sigmas=None):
    sn, sr = sigma_frames(case) if sigmas is None else sigmas
    return trans_psffit_ref(case['D'], case['N'], case['R'], sn, sr, case['mask'], case['pd'], case['ys'], case['xs'], case['scal'], SIZE, NSX,
                            case['W'], NITER, MAXSHIFT, dtype)
