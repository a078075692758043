"""The rules of the astrometric solution (include/bbx.h) stated in float64 numpy: the gnomonic projection about the
pointing and its inverse, the virtual grid, the catalogue as a star list, pixel to sky through T, the residual statistics, and
the whole solve as the chain of test_align_host.py (vote_ref, fit_ref, apply_ref).  No test lives here: test_astrometry_host.py
and test_gpu_astrometry.py import it.  Nothing of the package is imported."""
import numpy as np

F = np.float32
D2R, R2D = 0.017453292519943295, 57.29577951308232
POINTINGS = ((120.0, -30.0), (0.01, 89.2), (359.99, -5.0))


# ---- rule 1 --------------------------------------------------------------------------------------------------------
def std_of_sky(ra, dec, ra0, dec0):
    """(ra, dec) [deg] -> (xi, eta) [deg] about (ra0, dec0), and which rows are in the field"""
    ra, dec = np.asarray(ra, np.float64), np.asarray(dec, np.float64)
    with np.errstate(all='ignore'):
        da, d, d0 = (ra - ra0) * D2R, dec * D2R, dec0 * D2R
        sd, cd, sd0, cd0, sa, ca = np.sin(d), np.cos(d), np.sin(d0), np.cos(d0), np.sin(da), np.cos(da)
        D = sd0 * sd + cd0 * cd * ca
        xi, eta = (cd * sa / D) * R2D, ((cd0 * sd - sd0 * cd * ca) / D) * R2D
        ok = (D > 0.0) & np.isfinite(xi) & np.isfinite(eta)
    return xi, eta, ok


def sky_of_std(xi, eta, ra0, dec0):
    """(xi, eta) [deg] -> (ra in [0, 360), dec) [deg]"""
    with np.errstate(all='ignore'):
        x, e, d0 = np.asarray(xi, np.float64) * D2R, np.asarray(eta, np.float64) * D2R, dec0 * D2R
        sd0, cd0 = np.sin(d0), np.cos(d0)
        den = cd0 - e * sd0
        a = ra0 + np.arctan2(x, den) * R2D
        a = a - 360.0 * np.floor(a / 360.0)
        a = np.where(a >= 360.0, 0.0, a)
        dec = np.arctan2(sd0 + e * cd0, np.hypot(x, den)) * R2D
    return a, dec


def separation(ra1, dec1, ra2, dec2):
    """angular separation [deg], by the haversine form (exact for small angles, at the pole too)"""
    d1, d2 = np.asarray(dec1, np.float64) * D2R, np.asarray(dec2, np.float64) * D2R
    da = (np.asarray(ra1, np.float64) - np.asarray(ra2, np.float64)) * D2R
    h = np.sin(0.5 * (d1 - d2)) ** 2 + np.cos(d1) * np.cos(d2) * np.sin(0.5 * da) ** 2
    return 2.0 * np.arcsin(np.sqrt(np.minimum(h, 1.0))) * R2D


# ---- rule 2 --------------------------------------------------------------------------------------------------------
def cd0_of(pixscale, rot=0.0, parity=1):
    """CD0 [deg / pix], the FITS CROTA2 convention: parity +1 is north up, east left at rotation 0"""
    s, r, p = float(pixscale) / 3600.0, float(rot) * D2R, float(parity)
    return s * np.array([[-p * np.cos(r), -np.sin(r)], [-p * np.sin(r), np.cos(r)]], np.float64)


def grid_of_std(xi, eta, shape, cd):
    """(xi, eta) [deg] -> (x, y) on the virtual grid of a frame of [shape]: the closed-form inverse of CD0"""
    cd = np.asarray(cd, np.float64).reshape(4)
    with np.errstate(all='ignore'):
        det = cd[0] * cd[3] - cd[1] * cd[2]
        x = 0.5 * (shape[1] - 1) + (cd[3] * xi - cd[1] * eta) / det
        y = 0.5 * (shape[0] - 1) + (cd[0] * eta - cd[2] * xi) / det
    return x, y


# ---- rule 3 --------------------------------------------------------------------------------------------------------
def cat_list_ref(ra, dec, mag, pointing, shape, cd, margin, zp=25.0):
    """the catalogue as list B -> (ys, xs, off, flux, err), the eligible rows (bool), the float64 positions (x, y)"""
    mag = np.asarray(mag, F)
    xi, eta, ok = std_of_sky(ra, dec, *pointing)
    x, y = grid_of_std(xi, eta, shape, cd)
    with np.errstate(all='ignore'):
        ok = ok & np.isfinite(mag) & (x >= -margin) & (x <= shape[1] - 1 + margin) & (y >= -margin) & (y <= shape[0] - 1 + margin)
        flux = np.where(ok, 10.0 ** (-0.4 * (mag.astype(np.float64) - zp)), 0.0).astype(F)
        ok = ok & (flux > 0) & np.isfinite(flux)
    xs_, ys_ = np.where(ok, x, 0.0), np.where(ok, y, 0.0)
    fx, fy = np.floor(xs_ + 0.5), np.floor(ys_ + 0.5)
    off = np.where(ok[:, None], np.stack([ys_ - fy, xs_ - fx], axis=1), np.nan).astype(F)
    flux = np.where(ok, flux, F(0)).astype(F)
    return (fy.astype(np.int32), fx.astype(np.int32), off, flux, (flux / F(1000.0)).astype(F)), ok, (x, y)


# ---- rule 5 --------------------------------------------------------------------------------------------------------
def transform(coef, shape, x, y):
    """T at the frame position (x, y), bbx_align_grid's operations"""
    hy, hx = 0.5 * shape[0], 0.5 * shape[1]
    u, v = (np.asarray(x, np.float64) - hx) / hx, (np.asarray(y, np.float64) - hy) / hy
    b = [np.ones_like(u), u, v, u * u, u * v, v * v]
    X, Y = np.zeros_like(u), np.zeros_like(u)
    for t in range(6):
        X, Y = X + b[t] * coef[t], Y + b[t] * coef[6 + t]
    return X, Y


def pix2sky_ref(coef, shape, cd, pointing, x, y):
    cd = np.asarray(cd, np.float64).reshape(4)
    X, Y = transform(np.asarray(coef, np.float64), shape, x, y)
    dx, dy = X - 0.5 * (shape[1] - 1), Y - 0.5 * (shape[0] - 1)
    return sky_of_std(cd[0] * dx + cd[1] * dy, cd[2] * dx + cd[3] * dy, *pointing)


def list_positions(lst):
    """(x, y) float64 of a star list (ys, xs, off)"""
    off = np.asarray(lst[2], F).reshape(-1, 2)
    return np.asarray(lst[1]) + off[:, 1].astype(np.float64), np.asarray(lst[0]) + off[:, 0].astype(np.float64)


# ---- rule 6 --------------------------------------------------------------------------------------------------------
def pair_residuals(items, kept, a, cat_ra, cat_dec, coef, shape, cd, pointing, sky=None):
    """(dra cos dec, ddec) [arcsec] of the kept pairs, in item order, and their item indices; sky: (ra, dec) of every row of a
    where the caller has them already (else rule 5 here)"""
    items = np.asarray(items, np.int64).reshape(-1, 2)
    ia, ib = items[:, 0], items[:, 1]
    use = np.asarray(kept, bool) & (ia >= 0) & (ib >= 0) & (ia < len(a[0])) & (ib < len(cat_ra))
    idx = np.nonzero(use)[0]
    x, y = list_positions(a)
    ra, dec = pix2sky_ref(coef, shape, cd, pointing, x[ia[idx]], y[ia[idx]]) if sky is None else \
        (np.asarray(sky[0], np.float64)[ia[idx]], np.asarray(sky[1], np.float64)[ia[idx]])
    rc, dc = np.asarray(cat_ra, np.float64)[ib[idx]], np.asarray(cat_dec, np.float64)[ib[idx]]
    d = ra - rc
    d = d - 360.0 * np.floor((d + 180.0) / 360.0)
    return d * np.cos(dc * D2R) * 3600.0, (dec - dc) * 3600.0, idx


def ordered_sum(values, idx, block=256):
    """the kernel's order: thread t adds its items t, t + block, ... in that order, the partial sums are added in thread order"""
    part = np.zeros(block, np.float64)
    for v, i in zip(values.tolist(), idx.tolist()):
        part[i % block] += v
    tot = 0.0
    for p in part.tolist():
        tot += p
    return tot


def pair_stats_ref(items, kept, a, cat_ra, cat_dec, coef, shape, cd, pointing, sky=None):
    """-> [count, mean dra, std dra, mean ddec, std ddec]"""
    dra, ddec, idx = pair_residuals(items, kept, a, cat_ra, cat_dec, coef, shape, cd, pointing, sky)
    n = float(len(idx))
    if n == 0:
        return np.array([0.0, np.nan, np.nan, np.nan, np.nan])
    mra, mdec = ordered_sum(dra, idx) / n, ordered_sum(ddec, idx) / n
    return np.array([n, mra, np.sqrt(ordered_sum((dra - mra) * (dra - mra), idx) / n), mdec, np.sqrt(ordered_sum((ddec - mdec) * (ddec - mdec), idx) / n)])


# ---- rule 4: the whole solve ---------------------------------------------------------------------------------------
def solve_ref(a, ra, dec, mag, pointing, shape, cd, poldeg=2, max_shift=256.0, bin=4.0, rounds=3, dist=3.0, snr_min=15.0, zp=25.0, nmin=15,
              trace=None, b=None):
    """the chain of test_align_host.align_ref with B = the catalogue on the virtual grid -> its fit dict, with b (list B),
    n_eligible and stats (pair_stats_ref of the last fit's pairs).  b: list B where the caller has one to state the chain alone on
    (a list B from elsewhere may differ from cat_list_ref's in the last bit of a float32 offset)"""
    import test_align_host as A
    from test_match_host import match_mutual_ref
    b_ref, ok, _ = cat_list_ref(ra, dec, mag, pointing, shape, cd, max_shift + 16.0, zp)
    b = b_ref if b is None else b
    vt = A.vote_ref(a, b, max_shift=max_shift, bin=bin, nmin=nmin)
    fit = A.fit_ref(a, b, vt['pairs'], shape, 1, snr_min, nmin=nmin)
    items = vt['pairs']
    if trace is not None:
        trace.append((items, fit))
    for _ in range(rounds):
        s = A.sort_ref(*A.apply_ref(b[:3], fit['coef'], shape, poldeg))
        m = match_mutual_ref(a[0], a[1], a[2], s[0], s[1], s[2], dist)
        items = np.stack([np.where(m >= 0, np.arange(len(m)), -1), np.where(m >= 0, s[3][np.maximum(m, 0)], -1)], axis=1) \
            if len(m) and len(s[3]) else np.full((len(m), 2), -1)
        fit = A.fit_ref(a, b, items, shape, poldeg, snr_min, nmin=nmin)
        if trace is not None:
            trace.append((items, fit))
    flags = int(fit['flags']) | int(vt['info'][5])
    stats = pair_stats_ref(items, fit['kept'], a, ra, dec, fit['coef'], shape, cd, pointing) if np.isfinite(fit['coef']).all() else None
    return dict(fit, vote=vt, flags=flags, b=b, n_eligible=int(ok.sum()), items=items, stats=stats)


# ---- the toy of the issue: a true WCS that is not the nominal one --------------------------------------------------
def true_sky(x, y, shape, pointing, pixscale, tangent_offset=(0.01, 0.0), rot=0.3, scale=1.0007, quad=2e-6, parity=1):
    """the truth of a toy frame: frame pixels (x, y) -> sky through a TAN projection about a tangent point [tangent_offset] deg
    (east, north) away from the pointing, rotated and scaled against the nominal geometry, with a quadratic distortion of [quad] / px"""
    xc, yc = 0.5 * (shape[1] - 1), 0.5 * (shape[0] - 1)
    dx, dy = np.asarray(x, np.float64) - xc, np.asarray(y, np.float64) - yc
    dx, dy = dx + quad * (dx * dx - 0.5 * dx * dy), dy + quad * (dy * dy + 0.3 * dx * dy)
    cd = cd0_of(pixscale * scale, rot, parity)
    t_ra, t_dec = sky_of_std(tangent_offset[0], tangent_offset[1], *pointing)
    return sky_of_std(cd[0, 0] * dx + cd[0, 1] * dy, cd[1, 0] * dx + cd[1, 1] * dy, float(t_ra), float(t_dec))


def fit_truth(shape, pointing, cd, poldeg, sky_of_pixel, n=21):
    """the least-squares T of degree [poldeg] that maps frame pixels to the virtual-grid position of their true sky, on an n x n
    lattice over the frame -> coef [12], and the largest residual of the lattice in arcsec"""
    yy, xx = np.meshgrid(np.linspace(0, shape[0] - 1, n), np.linspace(0, shape[1] - 1, n), indexing='ij')
    x, y = xx.ravel(), yy.ravel()
    ra, dec = sky_of_pixel(x, y)
    xi, eta, ok = std_of_sky(ra, dec, *pointing)
    assert ok.all()
    X, Y = grid_of_std(xi, eta, shape, cd)
    hy, hx = 0.5 * shape[0], 0.5 * shape[1]
    u, v = (x - hx) / hx, (y - hy) / hy
    B = np.stack([np.ones_like(u), u, v, u * u, u * v, v * v], axis=1)[:, :6 if poldeg == 2 else 3]
    coef = np.zeros(12)
    coef[:B.shape[1]] = np.linalg.lstsq(B, X, rcond=None)[0]
    coef[6:6 + B.shape[1]] = np.linalg.lstsq(B, Y, rcond=None)[0]
    fra, fdec = pix2sky_ref(coef, shape, cd, pointing, x, y)
    return coef, float(separation(fra, fdec, ra, dec).max() * 3600.0)
