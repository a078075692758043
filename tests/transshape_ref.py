"""Transient vetting, the shape fits: the definition.  A numpy float64 restatement of bbx_trans_shapefit (include/bbx.h),
operation by operation, the cases the host tests (test_transshape_host.py) measure it on and the GPU tests (test_gpu_transshape.py)
compare the kernel with.

The window, its used pixels and V_D (float32) are bbx_trans_psffit's: transfit_ref.variance_d and the slicing of
transfit_ref.trans_psffit_ref, on transfit_ref's frame (make_case).  Everything behind the window is float64 by definition, so
there is no dtype argument; `order` is the order of the 36 sums over the window's pixels: 'fwd' (row-major) or 'rev'.  The kernel
has a third order (per lane over pixels lane, lane + 64, ..., then the wave), which the GPU test allows 4 x ORD_* for.

zogy's Gauss and Moffat fits to D are not in the reference tree: the rules are this project's own, parity is unpinned."""
import functools

import numpy as np

import psfphot_ref as PR
import transfit_ref as T

F = np.float32
AT_BOUND, MASKED, NO_FIT, NOT_CONVERGED, SHAPE_REFUSED = 1, 2, 4, 8, 16
GAUSS, MOFFAT = 1, 2
NPAR = 7                                                             # A, B, y0, x0, cyy, cxy, cxx
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX, STEP_TOL = 1e-3, 1e-9, 1e9, 0.01
NMIN = 8                                                             # used pixels a fit needs
OUT = ('dy', 'dx', 'dyerr', 'dxerr', 'fwhm', 'elong', 'chi2')        # the planes of d_out, in order
NITER, MAXSHIFT, BETA, FWHM_LO = 32, 2.0, 2.5, 0.5                  # settings.trans_shape_* / trans_moffat_beta

# ---- measured constants (CPU, numpy), each by the test named.
# pytest tests/test_transshape_host.py -k independent_minimiser -s
#   largest distance between the restatement's minimum and scipy.optimize.least_squares(method='lm') from the same start, over
#   the converged fits of truth_case(0 .. NSEED - 1) and CASES[1]: positions / the fit's own errors, FWHM, ELONG and chi2 relative
#   445 fits: 1.37e-4, 5.58e-5, 7.70e-5, 9.24e-10
LM_POS, LM_FWHM, LM_ELONG, LM_CHI2 = 1.4e-4, 5.6e-5, 7.7e-5, 9.3e-10
# pytest tests/test_transshape_host.py -k summation_order -s
#   largest change between order = 'fwd' and 'rev' over CASES, on the rows both orders mark converged: positions [pixel] / (W / 2),
#   errors, FWHM, ELONG, chi2 relative
#   1.77e-8, 2.12e-7 (W = 39, a fit that meets the step rule in its last iterations), 3.68e-8, 7.50e-8, 8.99e-15
ORD_POS, ORD_ERR, ORD_FWHM, ORD_ELONG, ORD_CHI2 = 1.8e-8, 2.2e-7, 3.7e-8, 7.6e-8, 9.0e-15
OUT_ROUND = 2.0 ** -22                                               # the float32 rounding of the kernel's outputs


def fin(v):
    return bool(abs(v) <= 1e300)                                     # (False for NaN)


def shape_k(model, beta):
    """FWHM of an axis = 2 sqrt(k / l), l the eigenvalue of the form"""
    return 2.0 * np.log(2.0) if model == GAUSS else 2.0 ** (1.0 / beta) - 1.0


def model_and_jacobian(model, beta, p, uy0, ux0):
    """m = B + A g(q), q = cyy dy^2 + 2 cxy dy dx + cxx dx^2 about (y0, x0) -> (m [n], J [7][n])"""
    A, B, y0, x0, cyy, cxy, cxx = p
    dy, dx = uy0 - y0, ux0 - x0
    q = cyy * dy * dy + 2.0 * cxy * dy * dx + cxx * dx * dx
    with np.errstate(all='ignore'):
        if model == GAUSS:
            g = np.exp(-0.5 * q)
            gq = -0.5 * g
        else:
            g = np.power(1.0 + q, -beta)
            gq = -beta * g / (1.0 + q)
        a = A * gq
        J = np.stack([g, np.ones_like(g), a * (-2.0 * (cyy * dy + cxy * dx)), a * (-2.0 * (cxy * dy + cxx * dx)), a * (dy * dy), a * (2.0 * dy * dx),
                      a * (dx * dx)])
        return B + A * g, J


def sums(model, beta, p, uy, ux, d, v):
    """the 28 + 7 + 1 sums at p: H = sum J J^T / V (upper triangle mirrored), g = sum J r / V, chi2 = sum r^2 / V"""
    m, J = model_and_jacobian(model, beta, p, uy, ux)
    with np.errstate(all='ignore'):
        r = d - m
        Jw = J / v
        H = J @ Jw.T
        H = np.triu(H) + np.triu(H, 1).T
        return H, (Jw * r).sum(axis=1), float((r * r / v).sum())


def cholesky(H, lam=0.0):
    """L of H + lam diag H, or None at a pivot that is not positive and finite"""
    L = np.zeros((NPAR, NPAR))
    with np.errstate(all='ignore'):
        for j in range(NPAR):
            s = H[j, j] * (1.0 + lam)
            for k in range(j):
                s -= L[j, k] * L[j, k]
            if not (s > 0 and s <= 1e300):
                return None
            L[j, j] = np.sqrt(s)
            for i in range(j + 1, NPAR):
                t = H[i, j]
                for k in range(j):
                    t -= L[i, k] * L[j, k]
                L[i, j] = t / L[j, j]
    return L


def chol_solve(L, b):
    x = np.zeros(NPAR)
    with np.errstate(all='ignore'):
        for i in range(NPAR):
            t = b[i]
            for k in range(i):
                t -= L[i, k] * x[k]
            x[i] = t / L[i, i]
        for i in range(NPAR - 1, -1, -1):
            t = x[i]
            for k in range(i + 1, NPAR):
                t -= L[k, i] * x[k]
            x[i] = t / L[i, i]
    return x


def chol_errors(L):
    """sqrt diag (L L^T)^-1: M = L^-1 column by column, diag_i = sum_k>=i M[k][i]^2"""
    e = np.zeros(NPAR)
    with np.errstate(all='ignore'):
        for i in range(NPAR):
            col = np.zeros(NPAR)
            col[i] = 1.0 / L[i, i]
            s = col[i] * col[i]
            for k in range(i + 1, NPAR):
                t = 0.0
                for j in range(i, k):
                    t -= L[k, j] * col[j]
                col[k] = t / L[k, k]
                s += col[k] * col[k]
            e[i] = np.sqrt(s)
    return e


def form_axes(model, beta, cyy, cxy, cxx):
    """-> (FWHM of the minor axis, of the major axis, l1, l2) or None where the form is not positive definite or not finite"""
    with np.errstate(all='ignore'):
        if not (fin(cyy) and fin(cxy) and fin(cxx)) or not (cyy > 0 and cxx > 0 and cyy * cxx - cxy * cxy > 0):
            return None
        hd = 0.5 * (cyy - cxx)
        root = np.sqrt(hd * hd + cxy * cxy)
        mean = 0.5 * (cyy + cxx)
        l1 = mean + root
        l2 = (cyy * cxx - cxy * cxy) / l1                            # (not mean - root: no cancellation)
        if not (l2 > 0 and fin(l1)):
            return None
        k = shape_k(model, beta)
        return 2.0 * np.sqrt(k / l1), 2.0 * np.sqrt(k / l2), l1, l2


def lm_fit(model, beta, uy, ux, d, v, p0, niter, bound, lo, hi):
    """Levenberg-Marquardt as bbx_trans_shapefit runs it -> (p, H, chi2, accepted, converged, shape_refused_last)"""
    p = np.array(p0, np.float64)
    H, g, chi2 = sums(model, beta, p, uy, ux, d, v)
    lam = LAMBDA0
    accepted = converged = shape_last = False
    for _ in range(niter):
        shape_last = False
        ok = False
        # a centre coordinate that sits at its bound while the gradient pushes it further out is held: its row and column leave the
        # system, so that the other parameters settle instead of chasing a step that the clamp takes back
        Hs, gs = H, g
        for i in (2, 3):
            if abs(p[i]) >= bound and g[i] * p[i] > 0:
                if Hs is H:
                    Hs, gs = H.copy(), g.copy()
                d_ii = Hs[i, i]
                Hs[i, :], Hs[:, i], gs[i] = 0.0, 0.0, 0.0
                Hs[i, i] = d_ii
        L = cholesky(Hs, lam)
        if L is not None:
            with np.errstate(all='ignore'):
                t = p + chol_solve(L, gs)
            ax = form_axes(model, beta, t[4], t[5], t[6]) if all(fin(x) for x in t) else None
            t[2], t[3] = min(max(t[2], -bound), bound), min(max(t[3], -bound), bound)
            if ax is None or not (ax[0] >= lo and ax[1] <= hi):
                shape_last = True
            else:
                Ht, gt, ct = sums(model, beta, t, uy, ux, d, v)
                ok = bool(fin(ct) and ct <= chi2)
        if ok:
            L0 = cholesky(H)
            if L0 is None:
                converged = False
            else:
                with np.errstate(all='ignore'):
                    converged = bool(np.all(np.abs(t - p) <= STEP_TOL * chol_errors(L0)))
            accepted = True
            p, H, g, chi2 = t, Ht, gt, ct
            lam = max(lam / 10.0, LAMBDA_MIN)
        else:
            lam = min(lam * 10.0, LAMBDA_MAX)
    return p, H, chi2, accepted, converged, shape_last


def window(D, N, R, sig_n, sig_r, mask, scal, size, nsx, nsy, y0, x0, W):
    """the window of bbx_trans_psffit at an on-frame peak -> (uy, ux (relative to the peak), d, v (float64 of the float32 values) over
    the used pixels in row-major order, masked?, D at the peak if it is used else None)"""
    ny, nx = D.shape
    hw = W // 2
    k = min(y0 // size, nsy - 1) * nsx + min(x0 // size, nsx - 1)
    ya, yb, xa, xb = max(y0 - hw, 0), min(y0 + hw + 1, ny), max(x0 - hw, 0), min(x0 + hw + 1, nx)
    wy, wx = np.mgrid[ya:yb, xa:xb]
    d = D[ya:yb, xa:xb].ravel()
    use = np.ones(d.shape, bool)
    masked = False
    if mask is not None:
        hit = mask[ya:yb, xa:xb].ravel() != 0
        masked = bool(hit.any())
        use &= ~hit
    use &= np.isfinite(d)
    with np.errstate(all='ignore'):
        v = T.variance_d(N[ya:yb, xa:xb].ravel(), R[ya:yb, xa:xb].ravel(), sig_n[ya:yb, xa:xb].ravel(), sig_r[ya:yb, xa:xb].ravel(), scal[k][2],
                         scal[k][3], np.float32)
        use &= (v > 0) & np.isfinite(v)
    uy, ux = (wy - y0).ravel()[use].astype(np.float64), (wx - x0).ravel()[use].astype(np.float64)
    peak = np.flatnonzero((uy == 0) & (ux == 0))
    d = d[use].astype(np.float64)
    return uy, ux, d, v[use].astype(np.float64), masked, (float(d[peak[0]]) if peak.size else None), k


def trans_shapefit_ref(D, N, R, sig_n, sig_r, mask, ys, xs, scal, fwhm0, size, nsx, W=11, niter=NITER, maxshift=MAXSHIFT, models=3, beta=BETA,
                       fwhm_lo=FWHM_LO, fwhm_hi=None, order='fwd'):
    """bbx_trans_shapefit.  Frames float32 [ny, nx] (sigma maps: frames), mask uint8 or None, scal [nsub, 6], fwhm0 [nsub] ->
    dict(out float64 [2][7][n] (planes OUT), flags uint8 [2][n], amp [2][n] (A, which the kernel does not write))"""
    D, N, R, sig_n, sig_r = (np.asarray(a, F) for a in (D, N, R, sig_n, sig_r))
    ny, nx = D.shape
    nsub = len(scal)
    nsy = nsub // nsx
    n = len(ys)
    out, flags, amp = np.zeros((2, NPAR, n)), np.zeros((2, n), np.uint8), np.zeros((2, n))
    bound = np.float64(F(maxshift))
    lo, hi = np.float64(F(fwhm_lo)), np.float64(F(2.0 * W if fwhm_hi is None else fwhm_hi))
    beta = np.float64(F(beta))
    for c in range(n):
        y0, x0 = int(ys[c]), int(xs[c])
        if y0 < 0 or y0 >= ny or x0 < 0 or x0 >= nx:
            flags[:, c] = NO_FIT
            continue
        uy, ux, d, v, masked, dpeak, k = window(D, N, R, sig_n, sig_r, mask, scal, size, nsx, nsy, y0, x0, W)
        fl = MASKED if masked else 0
        f0 = np.float64(F(fwhm0[k]))
        if len(d) < NMIN or not (f0 > 0 and fin(f0)):
            flags[:, c] = fl | NO_FIT
            continue
        f0 = min(max(f0, lo), hi)
        A0 = dpeak if dpeak is not None else float(d[np.argmax(np.abs(d))])      # (the first of equal |D| in row-major order)
        if order == 'rev':
            uy, ux, d, v = uy[::-1], ux[::-1], d[::-1], v[::-1]
        for mi, model in enumerate((GAUSS, MOFFAT)):
            if not models & model:
                flags[mi, c] = fl | NO_FIT
                continue
            c0 = 4.0 * shape_k(model, beta) / (f0 * f0)
            p, H, chi2, accepted, converged, shape_last = lm_fit(model, beta, uy, ux, d, v, (A0, 0.0, 0.0, 0.0, c0, 0.0, c0), niter, bound, lo, hi)
            L = cholesky(H)
            ax = form_axes(model, beta, p[4], p[5], p[6])
            if L is None or ax is None:
                flags[mi, c] = fl | NO_FIT
                continue
            e = chol_errors(L)
            with np.errstate(all='ignore'):
                res = (p[2], p[3], e[2], e[3], np.sqrt(ax[0] * ax[1]), np.sqrt(ax[2] / ax[3]), chi2 / (len(d) - NPAR))
            if not all(fin(x) for x in res):
                flags[mi, c] = fl | NO_FIT
                continue
            out[mi, :, c] = res
            amp[mi, c] = p[0]
            f = fl
            if abs(p[2]) >= bound or abs(p[3]) >= bound:
                f |= AT_BOUND
            if not accepted or not converged:
                f |= NOT_CONVERGED
            if shape_last:
                f |= SHAPE_REFUSED
            flags[mi, c] = f
    return dict(out=out, flags=flags, amp=amp)


# ---- the cases of the kernel tests --------------------------------------------------------------------------------------------
NY, NX, SIZE, NSY, NSX, NSUB, BOX = T.NY, T.NX, T.SIZE, T.NSY, T.NSX, T.NSUB, T.BOX
S_PD = 21                                                            # the stamps that make_case draws its sources with
# (W, ncand, sigma form, mask form, models, niter); ncand 1 and 65 leave a partly filled workgroup under four candidates per block.
# niter: the default but for W = 39, whose windows hold nine of the frame's sources (12 px apart): 61 of 65 Gauss fits have
# converged after 32 iterations, 65 of 65 after 64
CASES = ((5, 65, 'mini_x', 'zero', 3, NITER), (11, 300, 'frame', 'hits', 3, NITER), (39, 65, 'mini_c', None, 3, 64), (11, 1, 'frame', None, 2, NITER),
         (39, 1, 'mini_x', 'hits', 3, 64), (5, 65, 'mini_c', 'hits', 2, NITER), (11, 65, 'mini_x', None, 1, NITER))


def fwhm0_of(pd):
    """what the host hands the kernel: 2.3548 x zogy.window_sigma of the stamps, float32"""
    pd = np.asarray(pd, np.float64)
    return (2.3548 * np.sqrt(1.0 / (4.0 * np.pi * (pd * pd).sum(axis=(-2, -1))))).astype(F)


def make_case(W, ncand, sig_form, mask_form, models, niter=NITER):
    case = T.make_case(S_PD, W, ncand, sig_form, mask_form)
    case.update(models=models, niter=niter, fwhm0=fwhm0_of(case['pd']))
    return case


def run_case(case, order='fwd', sigmas=None, niter=None):
    sn, sr = T.sigma_frames(case) if sigmas is None else sigmas
    niter = case.get('niter', NITER) if niter is None else niter
    return trans_shapefit_ref(case['D'], case['N'], case['R'], sn, sr, case['mask'], case['ys'], case['xs'], case['scal'], case['fwhm0'], SIZE, NSX,
                              case['W'], niter, MAXSHIFT, case['models'], BETA, FWHM_LO, None, order)


@functools.lru_cache(maxsize=None)
def case_of(spec):
    case = make_case(*spec)
    return case, T.sigma_frames(case)


@functools.lru_cache(maxsize=None)
def case_run(spec, order='fwd'):
    """-> (case, the restatement in that order); computed once, shared by the host and the GPU tests"""
    case, sg = case_of(spec)
    return case, run_case(case, order, sg)


def case_runs(spec):
    """-> (case, the restatement in forward order, in reversed order)"""
    return case_run(spec, 'fwd') + (case_run(spec, 'rev')[1],)


# ---- injected sources of known shape ------------------------------------------------------------------------------------------
NSEED, W_TRUTH = 8, 11
KINDS = ('gauss', 'point', 'spike', 'dipole', 'trail')
N_KIND = dict(gauss=12, point=12, spike=4, dipole=3, trail=4)
FWHM_POINT, SIGMA_TRAIL, DIPOLE_HALF = 3.8, 1.6, 0.35


def truth_case(seed):
    """transfit_ref's frame with one source of its own (the corner's) and N_KIND sources of each kind injected into D alone (D's noise
    is that of V_D, which holds no source term here either) on every other cell of the 12-px grid, so that the nearest neighbour's
    centre lies 17 px away and nothing else in a window of 11:
      gauss   elliptical Gaussians, pixel-centre sampled (the model is exact): minor sigma 1.1 .. 1.3, axis ratio 1 .. 3, any angle,
              peak 25 .. 250 sigma, every other one negative
      point   Moffat (beta 2.5) of FWHM 3.8 -- not the model of either fit -- at S/N 8 .. 100, every other one negative
      spike   one pixel of 50 .. 125 sigma
      dipole  + and - the point source's profile 0.35 px either side of the cell, 10^5 e-
      trail   a straight segment of 15 px through the cell, Gaussian cross-section of sigma 1.6, peak 25 .. 60 sigma
    -> dict(case fields ..., kind [n], ys, xs, pos [n, 2] (true centre), sign [n], axes [n, 3] (sigma_major, sigma_minor, angle))"""
    case = T.make_case(S_PD, W_TRUTH, 1, 'frame', None, seed=50 + seed)
    rs = np.random.RandomState(900 + seed)
    gy, gx = np.mgrid[12:NY - 8:12, 12:NX - 4:12]
    cells = [(int(y), int(x)) for y, x in zip(gy.ravel(), gx.ravel()) if ((y + x) // 12) % 2 == 0]
    cells = [cells[i] for i in rs.permutation(len(cells))]
    kind = [k for k in KINDS for _ in range(N_KIND[k])]
    assert len(kind) <= len(cells)
    sg = T.sigma_frames(case)
    D = case['D'].astype(np.float64)
    yy, xx = np.mgrid[0:NY, 0:NX].astype(np.float64)
    pos, sign, axes = [], [], []
    for j, (kd, (y, x)) in enumerate(zip(kind, cells)):
        k = (y // SIZE) * NSX + x // SIZE
        fr = float(case['scal'][k][3])
        noise = float(np.sqrt(T.variance_d(*(np.asarray(a[y, x]) for a in (case['N'], case['R'], sg[0], sg[1])), 1.0, fr, np.float64)))
        oy, ox = rs.uniform(-0.5, 0.5, 2)
        sgn = -1.0 if j % 2 else 1.0
        ax = (0.0, 0.0, 0.0)
        if kd == 'gauss':
            smin = rs.uniform(1.1, 1.3)
            smaj, th = smin * rs.uniform(1.0, 3.0), rs.uniform(0, np.pi)
            u = (yy - y - oy) * np.sin(th) + (xx - x - ox) * np.cos(th)
            w = (yy - y - oy) * np.cos(th) - (xx - x - ox) * np.sin(th)
            D += sgn * noise * 10 ** rs.uniform(np.log10(25), np.log10(250)) * np.exp(-0.5 * (u * u / smaj ** 2 + w * w / smin ** 2))
            ax = (smaj, smin, th)
        elif kd == 'point':
            P = PR.moffat(FWHM_POINT, yy - y - oy, xx - x - ox)
            D += sgn * 10 ** rs.uniform(np.log10(8), 2) * noise / np.sqrt((P * P).sum()) * P
        elif kd == 'spike':
            oy = ox = 0.0
            sgn = 1.0
            D[y, x] += noise * rs.uniform(50, 125)
        elif kd == 'dipole':
            sgn = 1.0
            th = rs.uniform(0, 2 * np.pi)
            ey, ex = DIPOLE_HALF * np.sin(th), DIPOLE_HALF * np.cos(th)
            D += 1e5 * (PR.moffat(FWHM_POINT, yy - y - oy - ey, xx - x - ox - ex) - PR.moffat(FWHM_POINT, yy - y - oy + ey, xx - x - ox + ex))
        else:
            sgn = 1.0
            th = rs.uniform(0, np.pi)
            u = (yy - y - oy) * np.sin(th) + (xx - x - ox) * np.cos(th)
            w = (yy - y - oy) * np.cos(th) - (xx - x - ox) * np.sin(th)
            D += noise * rs.uniform(25, 60) * np.exp(-0.5 * w * w / SIGMA_TRAIL ** 2) * (np.abs(u) <= 7.5)
        pos.append((y + oy, x + ox)); sign.append(sgn); axes.append(ax)
    case['D'] = D.astype(F)
    n = len(kind)
    # the candidate is where the peak search would put it: the pixel of largest |D| within 2 px of the cell
    ys, xs = [], []
    for (y, x) in cells[:n]:
        w = np.abs(case['D'][y - 2:y + 3, x - 2:x + 3])
        iy, ix = np.unravel_index(int(np.argmax(w)), w.shape)
        ys.append(y - 2 + iy); xs.append(x - 2 + ix)
    case.update(ys=np.array(ys, np.int32), xs=np.array(xs, np.int32), kind=np.array(kind), pos=np.array(pos), sign=np.array(sign),
                axes=np.array(axes), models=3, W=W_TRUTH, fwhm0=fwhm0_of(case['pd']))
    return case


@functools.lru_cache(maxsize=None)
def truth_runs(seed):
    case = truth_case(seed)
    return case, run_case(case, 'fwd')
