"""numpy restatement of bbx_aper_phot (include/bbx.h): aperture photometry with a local sky annulus.  All geometry
in float64, the operations in the order the header states them, so that a pixel falls on the same side of every radius as in
the kernel; [dtype] is the type of the sums S, A, V (float64: the kernel's; float32: a twin that shows what single precision
would cost)."""
import numpy as np

NO_CENTROID, MASKED, OFF_FRAME, FEW_SKY, SKY_CUT, TOO_BIG = 1, 2, 4, 8, 16, 32
RMAX = 48.0                      # BBX_APER_RMAX
OFFMAX = 1.0e6                   # an offset beyond this is no centroid
F = np.float32


def _G(x, r, r2):
    """antiderivative of sqrt(r^2 - x^2)"""
    q = np.maximum(r2 - x * x, 0.0)
    t = np.minimum(np.maximum(x / r, -1.0), 1.0)
    return 0.5 * (x * np.sqrt(q) + r2 * np.arcsin(t))


def partial_area(ax, ay, r):
    """area of the disc of radius r about the origin inside the unit pixel centred on (ax, ay) (arrays, float64): the clipped chord
    height integrated over the pixel's x-range, split where the circle crosses the pixel's lower and upper edge"""
    ax, ay = np.asarray(ax, np.float64), np.asarray(ay, np.float64)
    r = np.float64(r)
    r2 = r * r
    x0, x1, y0, y1 = ax - 0.5, ax + 0.5, ay - 0.5, ay + 0.5
    a, b = np.maximum(x0, -r), np.minimum(x1, r)
    c0, c1 = np.sqrt(np.maximum(r2 - y0 * y0, 0.0)), np.sqrt(np.maximum(r2 - y1 * y1, 0.0))

    def clamp(v):
        return np.minimum(np.maximum(v, a), b)
    mid = np.sort(np.stack([clamp(-c0), clamp(c0), clamp(-c1), clamp(c1)]), axis=0)
    p = np.concatenate([a[None], mid, b[None]])
    g = _G(p, r, r2)
    area = np.zeros_like(ax)
    for i in range(5):
        lo, hi = p[i], p[i + 1]
        m = 0.5 * (lo + hi)
        h = np.sqrt(np.maximum(r2 - m * m, 0.0))
        arc = g[i + 1] - g[i]
        top = np.where(y1 <= h, y1 * (hi - lo), arc)
        bot = np.where(y0 >= -h, y0 * (hi - lo), -arc)
        on = (hi > lo) & (np.minimum(y1, h) > np.maximum(y0, -h))
        area = area + np.where(on, top - bot, 0.0)
    return np.minimum(np.maximum(area, 0.0), 1.0)             # (rounding may leave the sum a few 1e-17 outside)


def pixel_class(dy, dx, r):
    """-> (inside, touched): the farthest corner within r; the nearest point of the pixel within r"""
    ay, ax = np.abs(dy), np.abs(dx)
    r2 = np.float64(r) * np.float64(r)
    fy, fx = ay + 0.5, ax + 0.5
    far = fx * fx + fy * fy
    ny, nx = np.maximum(ay - 0.5, 0.0), np.maximum(ax - 0.5, 0.0)
    near = nx * nx + ny * ny
    return far <= r2, near < r2


def overlap_weights(dy, dx, r):
    """exact area of the disc of radius r inside the unit pixels whose centres lie at (dy, dx) from its centre"""
    dy, dx = np.asarray(dy, np.float64), np.asarray(dx, np.float64)
    inside, touched = pixel_class(dy, dx, r)
    w = np.where(inside, 1.0, 0.0)
    part = touched & ~inside
    if part.any():
        w[part] = partial_area(np.abs(dx[part]), np.abs(dy[part]), r)
    return w


def clip_stats(sample):
    """bbx_stats.h's rule on the float32 sample: 3 sigma about the exact median, population std, at most 5 rounds, stop when nothing
    is clipped -> (n, median, std) (NaN, NaN where n == 0)"""
    v = np.sort(np.asarray(sample, F)).astype(np.float64)
    lo, hi = 0, v.size
    med = std = np.nan
    for rnd in range(6):
        n = hi - lo
        if n == 0:
            break
        s = v[lo:hi]
        med = s[n // 2] if n & 1 else (s[n // 2 - 1] + s[n // 2]) / 2.0
        mean = s.sum() / n
        std = np.sqrt(((mean - s) ** 2).sum() / n)
        if rnd == 5:
            break
        nl = int((~(s >= med - 3.0 * std)).sum())
        nh = int(((s >= med - 3.0 * std) & ~(s <= med + 3.0 * std)).sum())
        if nl == 0 and nh == 0:
            break
        lo, hi = lo + nl, hi - nh
    n = hi - lo
    return (n, med, std) if n else (0, np.nan, np.nan)


def aper_phot_ref(D, sigma, mask, ys, xs, off, fwhm, size, nsy, nsx, radii=(0.66, 1.5, 5.0), sky_in=5.0, sky_out=7.0, sub_sky=True,
                  sky_nmin=20, dtype=np.float64):
    """-> dict(flux [n, naper], err [n, naper], sky [n, 3] = (median, std, n), flags uint8 [n]; float64, not yet rounded to float32;
    sumabs [n, naper] = sum of w |D| over the used pixels (the scale of the test's tolerance); closest = the smallest |d^2 - r^2|,
    |far - r^2|, |near - r^2| met at any radius (a comparison with the kernel is decisive only where this is well above the
    rounding of the geometry))"""
    D = np.asarray(D, F)
    sigma = np.asarray(sigma, F)
    ny, nx = D.shape
    ys, xs = np.asarray(ys), np.asarray(xs)
    n, naper = len(ys), len(radii)
    off = np.zeros((n, 2), F) if off is None else np.asarray(off, F)
    fwhm = np.asarray(fwhm, F).reshape(-1)
    rad = np.asarray(radii, F).astype(np.float64)
    flux, err = np.full((n, naper), np.nan), np.full((n, naper), np.nan)
    sky, flags = np.full((n, 3), np.nan), np.zeros(n, np.uint8)
    sumabs = np.zeros((n, naper))
    closest = np.inf
    for s in range(n):
        yp, xp = int(ys[s]), int(xs[s])
        oy, ox = np.float64(off[s, 0]), np.float64(off[s, 1])
        fl = 0
        if not (np.isfinite(oy) and np.isfinite(ox) and abs(oy) <= OFFMAX and abs(ox) <= OFFMAX):
            oy = ox = np.float64(0.0)
            fl |= NO_CENTROID
        f = fwhm[min(max(yp // size, 0), nsy - 1) * nsx + min(max(xp // size, 0), nsx - 1)]
        r = rad * np.float64(f)
        r_in, r_out = np.float64(F(sky_in)) * np.float64(f), np.float64(F(sky_out)) * np.float64(f)
        if not (np.isfinite(f) and f > 0 and r.max() <= RMAX and r_out <= RMAX):
            flags[s] = fl | TOO_BIG
            sky[s, 2] = 0.0
            continue
        R = max(r.max(), r_out)
        y_lo, y_hi = int(np.ceil(oy - R - 0.5)), int(np.floor(oy + R + 0.5))
        x_lo, x_hi = int(np.ceil(ox - R - 0.5)), int(np.floor(ox + R + 0.5))
        jy, jx = np.meshgrid(np.arange(y_lo, y_hi + 1), np.arange(x_lo, x_hi + 1), indexing='ij')
        dy, dx = jy.astype(np.float64) - oy, jx.astype(np.float64) - ox
        d2 = dy * dy + dx * dx
        iy, ix = yp + jy, xp + jx
        onf = (iy >= 0) & (iy < ny) & (ix >= 0) & (ix < nx)
        cy, cx = np.clip(iy, 0, ny - 1), np.clip(ix, 0, nx - 1)
        d, sg = D[cy, cx], sigma[cy, cx]
        used = onf & np.isfinite(d) & np.isfinite(sg)
        if mask is not None:
            used &= np.asarray(mask)[cy, cx] == 0
        d64 = d.astype(np.float64)
        var = (np.maximum(d, F(0)) + sg * sg).astype(np.float64)               # float32, as bbx_psf_optflux_sigma forms it
        # ---- the local sky
        ann = (d2 >= r_in * r_in) & (d2 < r_out * r_out)
        if (ann & ~used).any():
            fl |= SKY_CUT
        nsky, med, sd = clip_stats(d[ann & used])
        few = nsky < sky_nmin
        if few:
            fl |= FEW_SKY
        sky[s] = (np.nan, np.nan, nsky) if few else (med, sd, nsky)
        subtract = bool(sub_sky) and not few
        for rr in list(r) + [r_in, r_out]:
            closest = min(closest, np.abs(d2[used] - rr * rr).min(initial=np.inf))
        # ---- the apertures
        for k in range(naper):
            inside, touched = pixel_class(dy, dx, r[k])
            if (touched & ~onf).any():
                fl |= OFF_FRAME
            if (touched & onf & ~used).any():
                fl |= MASKED
            w = overlap_weights(dy, dx, r[k])
            ay, ax = np.abs(dy[used]), np.abs(dx[used])
            r2 = r[k] * r[k]
            closest = min(closest, np.abs((ax + 0.5) ** 2 + (ay + 0.5) ** 2 - r2).min(initial=np.inf),
                          np.abs(np.maximum(ax - 0.5, 0) ** 2 + np.maximum(ay - 0.5, 0) ** 2 - r2).min(initial=np.inf))
            wu = np.where(used, w, 0.0)
            S = (wu * d64)[used].astype(dtype).sum(dtype=dtype)
            A = wu[used].astype(dtype).sum(dtype=dtype)
            V = (wu * var)[used].astype(dtype).sum(dtype=dtype)
            sumabs[s, k] = (wu * np.abs(d64))[used].sum()
            S, A, V = np.float64(S), np.float64(A), np.float64(V)
            if A == 0:
                continue
            flux[s, k] = S - med * A if subtract else S
            err[s, k] = np.sqrt(V + (A * A * (np.pi / 2.0) * sd * sd / nsky if subtract else 0.0))
        flags[s] = fl
    return dict(flux=flux, err=err, sky=sky, flags=flags, sumabs=sumabs, closest=closest)
