"""The rules of bbx_limflux_image (include/bbx.h) restated in numpy: W and Q rounded to float32 exactly as the rules say, every sum
in float64.  Needs neither the library nor a reference tree."""
import numpy as np

F = np.float32


def moffat(S, fwhm, beta=2.5):
    """unit-sum float32 Moffat stamp of side S, centre S // 2"""
    a = fwhm / (2.0 * np.sqrt(2.0 ** (1.0 / beta) - 1.0))
    yy, xx = np.mgrid[0:S, 0:S] - S // 2
    p = (1.0 + (yy ** 2 + xx ** 2) / a ** 2) ** -beta
    return (p / p.sum()).astype(F)


def gauss(S, s):
    """unit-sum float32 Gaussian stamp of sigma s"""
    yy, xx = np.mgrid[0:S, 0:S] - S // 2
    p = np.exp(-(yy ** 2 + xx ** 2) / (2.0 * s * s))
    return (p / p.sum()).astype(F)


def q_stamp(plane):
    """rule 2 -> (Q float32 [S, S], ok)"""
    P = np.asarray(plane, F).astype(np.float64)
    norm = P.sum()
    if not (np.isfinite(norm) and norm > 0):
        return np.zeros(P.shape, F), False
    return ((P / norm) ** 2).astype(F), True


def central_sums(Q):
    """float64 sums of Q over the central T x T pixels, T = 1, 3, ..., S: ring by ring outwards -> array [S // 2 + 1]"""
    S = Q.shape[0]
    h = S // 2
    Q = Q.astype(np.float64)
    out, c = [], 0.0
    for m in range(h + 1):
        if m == 0:
            r = Q[h, h]
        else:
            r = Q[h - m, h - m:h + m + 1].sum() + Q[h + m, h - m:h + m + 1].sum() + Q[h - m + 1:h + m, h - m].sum() + Q[h - m + 1:h + m, h + m].sum()
        c += r
        out.append(c)
    return np.array(out)


def window(Q, frac):
    """rule 3 -> (T, margin): margin = the relative distance of the threshold from the sums at T and at T - 2, the smaller one
    (inf for frac == 0): a float64 summation order cannot move T while it stays far above 1e-16 x S^2"""
    S = Q.shape[0]
    if not 0.0 <= frac < 1.0:
        raise ValueError('frac in [0, 1) expected')
    if frac == 0.0:
        return S, np.inf
    cs = central_sums(Q)
    want = (1.0 - frac) * cs[-1]
    m = int(np.argmax(cs >= want))
    margin = (cs[m] - want) / want
    if m > 0:
        margin = min(margin, (want - cs[m - 1]) / want)
    return 2 * m + 1, float(margin)


def weights(sigma, mask):
    """rule 4 on the frame -> float32 [ny, nx]"""
    sigma = np.asarray(sigma, F)
    with np.errstate(all='ignore'):
        ok = np.isfinite(sigma) & (sigma > 0)
        W = np.where(ok, F(1.0) / (np.where(ok, sigma, F(1)) * np.where(ok, sigma, F(1))), F(0)).astype(F)
        W = np.minimum(W, np.finfo(F).max).astype(F)                   # sigma * sigma that underflows: the largest float32, not inf
    if mask is not None:
        W = np.where(np.asarray(mask) != 0, F(0), W).astype(F)
    return W


def tile_bounds(t, size, nt, n):
    """the pixels [lo, hi) of tile t of nt along an axis of n pixels (the clamp gives the rest to the last tile)"""
    lo = t * size
    hi = n if t == nt - 1 else min((t + 1) * size, n)
    return lo, max(hi, lo)


def limflux_ref(sigma, mask, planes, size, nsy, nsx, nsigma=5.0, frac=1e-4):
    """-> dict(lim float64 [ny, nx] (0 where den is not positive), den float64, win int32 [nsy * nsx], tmap int32 [ny, nx]: the
    window of every pixel's tile, margin: the smallest window margin of the tiles)"""
    W = weights(sigma, mask).astype(np.float64)
    ny, nx = W.shape
    planes = np.asarray(planes, F)
    S = planes.shape[1]
    h = S // 2
    Wp = np.zeros((ny + 2 * h, nx + 2 * h))
    Wp[h:h + ny, h:h + nx] = W
    den = np.zeros((ny, nx))
    tmap = np.zeros((ny, nx), np.int32)
    win = np.zeros(nsy * nsx, np.int32)
    margin = np.inf
    for ty in range(nsy):
        y0, y1 = tile_bounds(ty, size, nsy, ny)
        for tx in range(nsx):
            x0, x1 = tile_bounds(tx, size, nsx, nx)
            t = ty * nsx + tx
            Q, ok = q_stamp(planes[t])
            if not ok:
                continue
            T, mg = window(Q, frac)
            win[t], margin = T, min(margin, mg)
            if y1 <= y0 or x1 <= x0:
                continue
            k = T // 2
            tmap[y0:y1, x0:x1] = T
            Q64 = Q.astype(np.float64)
            acc = np.zeros((y1 - y0, x1 - x0))
            for j in range(-k, k + 1):
                for i in range(-k, k + 1):
                    acc += Q64[h + j, h + i] * Wp[h + y0 + j:h + y1 + j, h + x0 + i:h + x1 + i]
            den[y0:y1, x0:x1] = acc
    with np.errstate(all='ignore'):
        lim = np.where(den > 0, nsigma / np.sqrt(np.where(den > 0, den, 1.0)), 0.0)
    return dict(lim=lim, den=den, win=win, tmap=tmap, margin=margin)


def tile_windows(win, shape, size, nsy, nsx):
    """the window of every pixel's tile, int32 [ny, nx], from the tiles' windows"""
    gy, gx = np.mgrid[0:shape[0], 0:shape[1]]
    t = np.clip(gy // size, 0, nsy - 1) * nsx + np.clip(gx // size, 0, nsx - 1)
    return np.asarray(win, np.int32)[t]


def tolerance(T, mini=False):
    """relative bound of the float32 kernel against this restatement (tests/test_gpu_limflux.py's docstring); T: a window or an
    array of windows"""
    return (T * T / 2.0 + 8.0) * 2.0 ** -24 + (1e-6 if mini else 0.0)


def seam_planes(S, nsy, nsx, fwhm=(2.0, 5.68)):
    """the stamps of the GPU tests: neighbouring tiles get clearly different PSFs, Moffat FWHM 2.0 next to 5.68 (a checkerboard)"""
    return np.stack([moffat(S, fwhm[(t // nsx + t % nsx) % 2]) for t in range(nsy * nsx)])
