"""Flux ratio and dx, dy from matched stars, host side (no GPU): numpy restatements of the three kernels of
bbx_match.hip (include/bbx.h: bbx_win_centroid, bbx_match_mutual, bbx_match_stats) run on a synthetic scene with injected
per-tile flux ratios and astrometric scatter, and zogy.match_scalars / window_sigma, which are pure numpy.

The restatements are the definition the GPU tests (test_gpu_match.py) compare the kernels with; here they are checked
against the truth of the scene by conditions, not fitted numbers.
"""
import numpy as np
import pytest

F = np.float32
MATCH_CAP = 8192                    # BBX_MATCH_CAP


# ---- the restatements ----------------------------------------------------------------------------------------------
def win_centroid_ref(img, ys, xs, sigw, size, nsy, nsx, R, niter, dtype=np.float64):
    """bbx_win_centroid: -> [n, 2] (dy, dx) relative to the integer peak, NaN where there is none; dtype: the arithmetic"""
    img = np.asarray(img)
    ny, nx = img.shape
    out = np.full((len(ys), 2), np.nan, dtype)
    gy, gx = np.mgrid[-R:R + 1, -R:R + 1]
    py, px = gy.ravel().astype(dtype), gx.ravel().astype(dtype)
    for k, (yc, xc) in enumerate(zip(ys, xs)):
        yy, xx = yc + gy.ravel(), xc + gx.ravel()
        on = (yy >= 0) & (yy < ny) & (xx >= 0) & (xx < nx)
        I = np.zeros(py.size, dtype)
        I[on] = img[yy[on], xx[on]].astype(dtype)
        sg = dtype(sigw[min(max(yc // size, 0), nsy - 1) * nsx + min(max(xc // size, 0), nsx - 1)])
        with np.errstate(all='ignore'):
            inv = dtype(1) / (dtype(2) * sg * sg)
            ok = bool(sg > 0 and np.isfinite(sg) and np.isfinite(inv))
            cy = cx = dtype(0)
            for _ in range(niter):
                if not ok:
                    break
                dy, dx = py - cy, px - cx
                w = np.exp(-(dy * dy + dx * dx) * inv).astype(dtype) * I
                sw, sy, sx = w.sum(dtype=dtype), (w * dy).sum(dtype=dtype), (w * dx).sum(dtype=dtype)
                ok = bool(sw > 0 and np.isfinite(sw) and np.isfinite(sy) and np.isfinite(sx))
                if ok:
                    cy, cx = cy + dtype(2) * (sy / sw), cx + dtype(2) * (sx / sw)
                    ok = bool(np.isfinite(cy) and np.isfinite(cx) and abs(cy) <= dtype(0.5) * dtype(R) and abs(cx) <= dtype(0.5) * dtype(R))
        if ok:
            out[k] = cy, cx
    return out


def match_mutual_ref(a_ys, a_xs, a_off, b_ys, b_xs, b_off, dist_max):
    """bbx_match_mutual by brute force: float32 distances, inclusive radius, band of ceil(dist_max + 1) rows and columns,
    ties to the lower index, NaN offsets match nothing -> int32 [n_a]"""
    n_a, n_b = len(a_ys), len(b_ys)
    if n_a == 0 or n_b == 0:
        return np.full(n_a, -1, np.int32)
    a_off, b_off = np.asarray(a_off, F), np.asarray(b_off, F)
    band = int(np.ceil(F(dist_max) + F(1)))
    iy = np.asarray(b_ys, np.int64)[None, :] - np.asarray(a_ys, np.int64)[:, None]
    ix = np.asarray(b_xs, np.int64)[None, :] - np.asarray(a_xs, np.int64)[:, None]
    with np.errstate(invalid='ignore'):
        dy = iy.astype(F) + (b_off[None, :, 0] - a_off[:, None, 0])
        dx = ix.astype(F) + (b_off[None, :, 1] - a_off[:, None, 1])
        d2 = dy * dy + dx * dx
        ok = (d2 <= F(dist_max) * F(dist_max)) & (np.abs(iy) <= band) & (np.abs(ix) <= band)
    d2 = np.where(ok, d2, np.inf)
    best_b = np.where(ok.any(axis=1), d2.argmin(axis=1), -1)          # argmin: the first (lowest) index of the minimum
    best_a = np.where(ok.any(axis=0), d2.argmin(axis=0), -1)
    a = np.arange(n_a)
    return np.where((best_b >= 0) & (best_a[np.maximum(best_b, 0)] == a), best_b, -1).astype(np.int32)


def clip_ref(vals):
    """oracle/zogy_core.box_stats on float32 values in float64, also returning who survives
    -> (n, median, mean, std, keep)"""
    vals = np.asarray(vals, F).astype(np.float64)
    keep = np.ones(vals.size, bool)
    for _ in range(5):
        v = vals[keep]
        if v.size == 0:
            break
        med, mean = np.median(v), v.sum() / v.size
        std = np.sqrt(((mean - v) ** 2).sum() / v.size)
        k2 = keep & (vals >= med - 3.0 * std) & (vals <= med + 3.0 * std)
        if k2.sum() == keep.sum():
            break
        keep = k2
    v = vals[keep]
    if v.size == 0:
        return 0, np.nan, np.nan, np.nan, keep
    mean = v.sum() / v.size
    return v.size, np.median(v), mean, np.sqrt(((v - mean) ** 2).sum() / v.size), keep


def match_stats_ref(a, b, match, size, nsy, nsx, snr_min, cap=MATCH_CAP):
    """bbx_match_stats: a, b = (ys, xs, off, flux, err) -> float64 [nsy * nsx + 1, 16]"""
    a_ys, a_xs, a_off, a_f, a_e = [np.asarray(t) for t in a]
    b_ys, b_xs, b_off, b_f, b_e = [np.asarray(t) for t in b]
    nsub = nsy * nsx
    out = np.full((nsub + 1, 16), np.nan)
    out[:, [0, 1, 7, 11]] = 0.0
    out[:, 15] = 1.0
    match = np.asarray(match)
    m = np.maximum(match, 0)
    if len(a_ys) == 0:
        return out
    if len(b_ys) == 0:
        b_ys = b_xs = np.zeros(1, np.int32); b_off = np.zeros((1, 2), F); b_f = b_e = np.zeros(1, F)
    fa, ea, fb, eb = a_f.astype(F), a_e.astype(F), b_f.astype(F)[m], b_e.astype(F)[m]
    with np.errstate(all='ignore'):
        q = (match >= 0) & (fa > 0) & (fb > 0) & (fa / ea >= F(snr_min)) & (fb / eb >= F(snr_min))
        fr = (fa / fb).astype(F)
        dx = (a_xs - b_xs[m]).astype(F) + (a_off[:, 1].astype(F) - b_off[m, 1].astype(F))
        dy = (a_ys - b_ys[m]).astype(F) + (a_off[:, 0].astype(F) - b_off[m, 0].astype(F))
        sig = fr.astype(np.float64) * np.sqrt((ea.astype(np.float64) / fa) ** 2 + (eb.astype(np.float64) / fb) ** 2)
    for seg in range(nsub + 1):
        if seg < nsub:
            ty, tx = divmod(seg, nsx)
            inside = (a_ys >= ty * size) & (a_ys < (ty + 1) * size) & (a_xs >= tx * size) & (a_xs < (tx + 1) * size)
        else:
            inside = np.ones(len(a_ys), bool)
        idx = np.nonzero(q & inside)[0]
        n = idx.size
        if n == 0:
            continue
        s = -(-n // cap) if n > cap else 1
        idx = idx[::s]
        row = out[seg]
        row[0], row[15] = n, s
        row[1:5] = clip_ref(fr[idx])[:4]
        keep = clip_ref(fr[idx])[4]
        w = 1.0 / sig[idx][keep] ** 2
        row[5], row[6] = (w * fr[idx][keep].astype(np.float64)).sum() / w.sum(), 1.0 / np.sqrt(w.sum())
        row[7:11] = clip_ref(dx[idx])[:4]
        row[11:15] = clip_ref(dy[idx])[:4]
    return out


# ---- the scene -----------------------------------------------------------------------------------------------------
SIZE, NSY, NSX = 120, 2, 4
NY, NX = NSY * SIZE, NSX * SIZE
RATIOS = np.array([0.6, 0.7, 0.8, 0.9, 1.0, 1.1, 1.25, 1.4])         # injected per tile, all >= 0.1 apart
FWHM_REF, FWHM_NEW, SKY_REF, SKY_NEW = 3.0, 3.6, 6.0, 14.0
BETA, PSF_S = 2.5, 25
SHIFT = (-0.01, 0.02)                                               # constant offset new - ref (y, x)
SCATTER = (0.03, 0.06)                                              # sigma of the positional scatter (y, x)
CAT_NSIGMA, SNR_MIN, DIST, NMIN, RAD, NITER = 5.0, 20.0, 3.5, 15, 6, 8


def moffat(fwhm, yy, xx):
    alpha = fwhm / (2.0 * np.sqrt(2.0 ** (1.0 / BETA) - 1.0))
    return (BETA - 1.0) / (np.pi * alpha ** 2) * (1.0 + (yy * yy + xx * xx) / alpha ** 2) ** (-BETA)


def psf_stamp(fwhm, S=PSF_S):
    g = np.arange(S) - S // 2
    p = moffat(fwhm, g[:, None].astype(np.float64), g[None, :].astype(np.float64))
    return (p / p.sum()).astype(F)


def render(ny, nx, ys, xs, flux, fwhm, half=15):
    img = np.zeros((ny, nx))
    for y, x, f in zip(ys, xs, flux):
        y0, x0 = int(round(y)), int(round(x))
        ya, yb, xa, xb = max(y0 - half, 0), min(y0 + half + 1, ny), max(x0 - half, 0), min(x0 + half + 1, nx)
        gy, gx = np.mgrid[ya:yb, xa:xb]
        img[ya:yb, xa:xb] += f * moffat(fwhm, gy - y, gx - x)
    return img


def make_scene(seed=5, nstars=None):
    """-> dict: background-subtracted float32 frames new, ref (zero-mean noise), the truth of the stars, the PSF stamps"""
    rs = np.random.RandomState(seed)
    gy, gx = np.meshgrid(10 + 19.5 * np.arange(12), 10 + 19.2 * np.arange(25), indexing='ij')
    ry = gy.ravel() + rs.uniform(-3, 3, gy.size)
    rx = gx.ravel() + rs.uniform(-3, 3, gx.size)
    if nstars is not None:
        pick = rs.permutation(ry.size)[:nstars]
        ry, rx = ry[pick], rx[pick]
    f_ref = 10 ** rs.uniform(4.0, np.log10(2e5), ry.size)
    ny_ = ry + SHIFT[0] + rs.normal(0, SCATTER[0], ry.size)
    nx_ = rx + SHIFT[1] + rs.normal(0, SCATTER[1], ry.size)
    tile = (np.clip(ry // SIZE, 0, NSY - 1) * NSX + np.clip(rx // SIZE, 0, NSX - 1)).astype(int)
    f_new = f_ref * RATIOS[tile]
    ref = render(NY, NX, ry, rx, f_ref, FWHM_REF)
    new = render(NY, NX, ny_, nx_, f_new, FWHM_NEW)
    ref = ref + rs.normal(0, 1, ref.shape) * np.sqrt(ref + SKY_REF ** 2)      # Poisson (Gaussian limit) + sky noise
    new = new + rs.normal(0, 1, new.shape) * np.sqrt(new + SKY_NEW ** 2)
    return dict(new=new.astype(F), ref=ref.astype(F), ry=ry, rx=rx, ny=ny_, nx=nx_, f_ref=f_ref, f_new=f_new, tile=tile,
                psf_new=psf_stamp(FWHM_NEW), psf_ref=psf_stamp(FWHM_REF))


def host_peaks(img, thr):
    """bbx_find_peaks: per 8-connected region of |img| >= thr the pixel of largest |value|; sorted by (y, x), peaks > 0"""
    from scipy import ndimage
    lab, n = ndimage.label(np.abs(img) >= thr, structure=np.ones((3, 3)))
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    pos = np.array(ndimage.maximum_position(np.abs(img), lab, np.arange(1, n + 1)))
    pos = pos[img[pos[:, 0], pos[:, 1]] > 0]
    o = np.lexsort((pos[:, 1], pos[:, 0]))
    return pos[o, 0].astype(np.int32), pos[o, 1].astype(np.int32)


def host_optflux(img, sigma, psf, ys, xs):
    """zogy.get_psfoptflux at integer positions: V = max(D, 0) + sigma^2; pixels off the frame are skipped"""
    S = psf.shape[0]
    h = S // 2
    ny, nx = img.shape
    f, e = np.zeros(len(ys), F), np.zeros(len(ys), F)
    for k, (y, x) in enumerate(zip(ys, xs)):
        ya, yb, xa, xb = max(y - h, 0), min(y + h + 1, ny), max(x - h, 0), min(x + h + 1, nx)
        P = psf[ya - (y - h):yb - (y - h), xa - (x - h):xb - (x - h)].astype(np.float64)
        D = img[ya:yb, xa:xb].astype(np.float64)
        V = np.maximum(D, 0) + sigma ** 2
        f[k], e[k] = (P * D / V).sum() / (P * P / V).sum(), 1.0 / np.sqrt((P * P / V).sum())
    return f, e


def host_catalog(img, sigma, psf, dtype=np.float64):
    from blackbox_amd import zogy as G
    ys, xs = host_peaks(img, CAT_NSIGMA * sigma)
    f, e = host_optflux(img, sigma, psf, ys, xs)
    sw = np.full(NSY * NSX, G.window_sigma(psf))
    off = win_centroid_ref(img, ys, xs, sw, SIZE, NSY, NSX, RAD, NITER, dtype)
    return ys, xs, off.astype(F), f, e


@pytest.fixture(scope='module')
def measured():
    sc = make_scene()
    a = host_catalog(sc['new'], SKY_NEW, sc['psf_new'])
    b = host_catalog(sc['ref'], SKY_REF, sc['psf_ref'])
    match = match_mutual_ref(a[0], a[1], a[2], b[0], b[1], b[2], DIST)
    return sc, a, b, match, match_stats_ref(a, b, match, SIZE, NSY, NSX, SNR_MIN)


# ---- tests ---------------------------------------------------------------------------------------------------------
def test_restatement_recovers_the_injected_ratios_and_scatter(measured):
    from blackbox_amd import zogy as G
    sc, a, b, match, table = measured
    nsub = NSY * NSX
    ms = G.match_scalars(table, 1.0, 0.0, 0.0, NMIN)
    print('sources new %d, ref %d, pairs %d, qualifying %d (per tile %s)' % (len(a[0]), len(b[0]), (match >= 0).sum(), table[nsub, 0],
                                                                             table[:nsub, 0].astype(int).tolist()))
    print('per-tile ratio - injected:', np.round(ms['fratio_sub'] - RATIOS, 4).tolist())
    full = dict(zip(G.MATCH_COLS, table[nsub]))
    print('full frame: dx med %+.4f std %.4f (injected %+.2f, %.2f); dy med %+.4f std %.4f (injected %+.2f, %.2f); fr med %.4f '
          'std %.4f werr %.5f' % (full['med_dx'], full['std_dx'], SHIFT[1], SCATTER[1], full['med_dy'], full['std_dy'], SHIFT[0],
                                  SCATTER[0], full['med_fr'], full['std_fr'], full['werr_fr']))
    assert ms['success'] and (table[:nsub, 1] >= NMIN).all()
    # every tile's ratio is nearer its own injected value than any other tile's
    for k in range(nsub):
        assert np.abs(ms['fratio_sub'][k] - RATIOS).argmin() == k, (k, ms['fratio_sub'][k])
    assert full['std_dx'] > full['std_dy']
    assert full['med_dx'] > 0 and full['med_dy'] < 0
    assert ms['header']['Z-FNRERR'][0] == full['werr_fr'] and ms['header']['Z-DXSTD'][0] == full['std_dx']


def test_float32_centroid_follows_float64(measured):
    sc, a, _, _, _ = measured
    from blackbox_amd import zogy as G
    sw = np.full(NSY * NSX, G.window_sigma(sc['psf_new']))
    c64 = win_centroid_ref(sc['new'], a[0], a[1], sw, SIZE, NSY, NSX, RAD, NITER, np.float64)
    c32 = win_centroid_ref(sc['new'], a[0], a[1], sw, SIZE, NSY, NSX, RAD, NITER, np.float32)
    assert np.array_equal(np.isnan(c64), np.isnan(c32))
    d = np.nanmax(np.abs(c64 - c32))
    print('float32 against float64 centroid: max difference %.3g px over %d sources' % (d, len(a[0])))


def table_with(counts, nsub=4):
    """a table whose rows differ: tile k has ratio 1 + 0.1 k, mean_dx 0.01 k, std_dx 0.05, ...; the full-frame row 2.0"""
    from blackbox_amd import zogy as G
    t = G.empty_match_table(nsub)
    c = {k: i for i, k in enumerate(G.MATCH_COLS)}
    for k in range(nsub + 1):
        n = counts[k]
        t[k, [c['n_qualifying'], c['n_fr'], c['n_dx'], c['n_dy']]] = n
        if n:
            t[k, c['med_fr']] = 2.0 if k == nsub else 1.0 + 0.1 * k
            t[k, c['mean_dx']], t[k, c['std_dx']], t[k, c['med_dx']] = 0.01 * k, 0.05, 0.011 * k
            t[k, c['mean_dy']], t[k, c['std_dy']], t[k, c['med_dy']] = -0.02 * k, 0.03, -0.021 * k
            t[k, c['std_fr']], t[k, c['werr_fr']] = 0.04, 0.002
    return t


def test_match_scalars_thresholds():
    from blackbox_amd import zogy as G
    nmin = 15
    t = table_with([nmin - 1, nmin, 0, 40, 100])
    ms = G.match_scalars(t, 0.9, 0.03, 0.02, nmin)
    assert ms['success']
    full_dx, full_dy = np.hypot(0.04, 0.05), np.hypot(-0.08, 0.03)
    # below nmin (and empty): the full-frame values; exactly nmin: its own
    assert np.allclose(ms['fratio_sub'], [2.0, 1.1, 2.0, 1.3], rtol=0, atol=1e-15)
    assert np.allclose(ms['dx_sub'], [full_dx, np.hypot(0.01, 0.05), full_dx, np.hypot(0.03, 0.05)], rtol=0, atol=1e-15)
    assert np.allclose(ms['dy_sub'], [full_dy, np.hypot(-0.02, 0.03), full_dy, np.hypot(-0.06, 0.03)], rtol=0, atol=1e-15)
    h = ms['header']
    assert list(h) == ['Z-DX', 'Z-DY', 'Z-DXSTD', 'Z-DYSTD', 'Z-FNR', 'Z-FNRSTD', 'Z-FNRERR']
    assert (h['Z-DX'][0], h['Z-DY'][0], h['Z-DXSTD'][0], h['Z-DYSTD'][0]) == (0.011 * 4, -0.021 * 4, 0.05, 0.03)
    assert (h['Z-FNR'][0], h['Z-FNRSTD'][0], h['Z-FNRERR'][0]) == (2.0, 0.04, 0.002)
    assert h['Z-FNRERR'][1] == 'weighted error flux ratio (Fnew/Fref) full image'


def test_match_scalars_without_enough_pairs_keeps_the_callers_numbers():
    from blackbox_amd import zogy as G
    t = table_with([3, 4, 0, 5, 12])                                 # full-frame row below nmin
    ms = G.match_scalars(t, 0.9, 0.03, 0.02, 15)
    assert ms['success'] is False
    assert np.array_equal(ms['fratio_sub'], np.full(4, 0.9)) and np.array_equal(ms['dx_sub'], np.full(4, 0.03))
    assert np.array_equal(ms['dy_sub'], np.full(4, 0.02))
    h = ms['header']
    assert (h['Z-DX'][0], h['Z-DY'][0], h['Z-FNR'][0]) == (0.03, 0.02, 0.9)
    assert [h[k][0] for k in ('Z-DXSTD', 'Z-DYSTD', 'Z-FNRSTD', 'Z-FNRERR')] == ['None'] * 4
    # one number per tile from the caller stays one per tile
    per = np.array([0.8, 0.9, 1.0, 1.1])
    ms = G.match_scalars(G.empty_match_table(4), per, 0.0, 0.0, 15)
    assert not ms['success'] and np.array_equal(ms['fratio_sub'], per) and ms['header']['Z-FNR'][0] == 0.95


def test_window_sigma_of_a_gaussian_stamp():
    from blackbox_amd import zogy as G
    g = np.arange(25) - 12
    p = np.exp(-(g[:, None] ** 2 + g[None, :] ** 2) / (2 * 2.0 ** 2))
    p /= p.sum()
    assert abs(G.window_sigma(p) / 2.0 - 1) <= 1e-3
    assert G.window_sigma(np.stack([p, p])).shape == (2,)


def test_settings_defaults():
    from blackbox_amd import settings as S
    assert S.zogy_match is False
    assert (S.match_dist_pix, S.match_nmin, S.match_snr_min, S.centroid_radius, S.centroid_niter) == (3.5, 15, 20.0, 6, 8)


def test_library_rejects_bad_arguments_without_gpu():
    from blackbox_amd import _lib
    L = _lib.lib
    assert L.bbx_win_centroid(None, 10, 10, None, 1, None, None, None, 5, 2, 2, 6, 8, None, None) == -1
    assert L.bbx_match_mutual(None, 1, None, None, None, 1, None, None, None, 3.5, None, None, None) == -1
    assert L.bbx_match_stats(None, 1, None, None, None, None, None, 1, None, None, None, None, None, None, 5, 2, 2, 20.0, None, None) == -1
